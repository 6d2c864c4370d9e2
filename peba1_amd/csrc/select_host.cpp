// select_host.cpp -- host side of the private selection: the TGSW encryption of index bits, the selector object and the
// C ABI of the CMUX tree and of the packed lookup (include/tfhe_hip.h "private selection", "private lookup").  The negacyclic product is pack_host.cpp's.  No arithmetic
// of the CMUX itself happens here (cmux.hip); encryption runs on the CPU like that of the ring samples.
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

// (struct TfheHipSelector: shim_internal.hpp -- seeded_select_host.cpp makes the compressed kind)

namespace {
constexpr uint32_t SELECT_MAGIC = 0x53454C54u;
// the most CMUXes one raw launch takes (tfhe_hip_kernel_ring_cmux)
constexpr int32_t CMUX_MAX_COUNT = 1 << 16;

// The draw order (include/tfhe_hip.h): for every bit, for u <= k, for p < l: the kN mask words, then the N noise samples
// -- the order of the bootstrapping key's rows (host_keys.cpp generate_keys), of which a selector bit is one entry.
// polys false: sample b encrypts the bit bits[b] (a constant polynomial); true: the polynomial at bits[b N .. + N)
void tgsw_encrypt_into(const TfheHipSecretKey &sk, const int32_t *bits, bool polys, int32_t count, Rng &secret, Rng &mask, Torus32 *out) {
    const Params &p = sk.p;
    const int N = p.N, k = p.k, l = p.l, kpl = p.kpl();
    for (int32_t b = 0; b < count; ++b)
        for (int row = 0; row < kpl; ++row) {
            uint32_t *smp = reinterpret_cast<uint32_t *>(out) + ((size_t)b * kpl + row) * (size_t)(k + 1) * N;
            uint32_t *body = smp + (size_t)k * N;
            for (int u = 0; u < k; ++u)
                for (int j = 0; j < N; ++j) smp[(size_t)u * N + j] = (uint32_t)mask.torus();
            for (int j = 0; j < N; ++j) body[j] = (uint32_t)dtot32(secret.gauss(p.bk_stdev));
            for (int u = 0; u < k; ++u) pack_add_mul_by_bits(body, smp + (size_t)u * N, sk.tlwe_key.data() + (size_t)u * N, N, 1u);
            const int u = row / l, pp = row % l;
            const int shift = 32 - (pp + 1) * p.Bgbit;
            if (!polys) smp[(size_t)u * N] += (uint32_t)(bits[b] ? 1 : 0) << shift;
            else
                for (int j = 0; j < N; ++j) smp[(size_t)u * N + j] += (uint32_t)bits[(size_t)b * N + j] << shift;
        }
}

int tgsw_encrypt_impl(const char *who, const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                      Torus32 *out, const uint64_t *seed, bool polys = false) {
    if (!secret || !secret->lwe_key || !bits || !out) { set_error(std::string(who) + ": null argument"); return -1; }
    if (count < 1 || count > SELECT_MAX_BITS) {
        set_error(std::string(who) + ": count must be in 1.." + std::to_string(SELECT_MAX_BITS));
        return -1;
    }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    if (seed) {
        Rng both(*seed);                                  // a stream of its own, for this selector alone
        tgsw_encrypt_into(sk, bits, polys, count, both, both, out);
    } else {
        Rng noise = Rng::secure(), mask = Rng::secure();  // two fresh ChaCha20 streams, as for a ring sample
        tgsw_encrypt_into(sk, bits, polys, count, noise, mask, out);
    }
    return 0;
}

int select_impl(const char *who, const TfheHipSelector *sel, const Torus32 *ring, int32_t M, Torus32 *out, bool on_device) {
    const std::string w = std::string(who) + ": ";
    selector_checked(w, sel);
    if (!ring || !out) api_fail(w + "null ring words or destination");
    if (M < 1 || (int64_t)M > ((int64_t)1 << sel->nbits))
        api_fail(w + "M must be in 1..2^" + std::to_string(sel->nbits) + " for a selector of " + std::to_string(sel->nbits) + " bits");
    // (the kernel loads and stores 16 bytes at a time)
    if (on_device && ((reinterpret_cast<uintptr_t>(ring) | reinterpret_cast<uintptr_t>(out)) & 15))
        api_fail(w + "device words must be 16-byte aligned");
    auto g = recorder_lock();
    // names no pool slot: what is recorded stays recorded, a flush in flight goes on (the select is ordered behind it on
    // the stream and works in scratch entries of its own)
    const RingImage *img = select_image(sel);     // out of device memory: ApiError, nothing has changed
    Engine::get().run_select(img, sel->p, sel->nbits, ring, M, on_device, out, on_device);
    return 0;
}

// the packed lookup: every argument before the device is looked at, in the order the header lists the refusals
int lookup_impl(const char *who, const TfheHipSelector *sel, const Torus32 *ring, int32_t M, int32_t width, Torus32 *out, bool on_device) {
    const std::string w = std::string(who) + ": ";
    selector_checked(w, sel);
    if (!ring || !out) api_fail(w + "null ring words or destination");
    const int N = sel->p.N;
    if (width < 1 || width > N || (width & (width - 1)))
        api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
    int s = 0;
    while ((width << s) < N) ++s;
    if (sel->nbits < s)
        api_fail(w + "entries of width " + std::to_string(width) + " need the " + std::to_string(s) + " rotation bits of a sample; the selector has " +
                 std::to_string(sel->nbits) + " bits");
    if (M < 1 || (int64_t)M > ((int64_t)1 << sel->nbits))
        api_fail(w + "M must be in 1..2^" + std::to_string(sel->nbits) + " for a selector of " + std::to_string(sel->nbits) + " bits");
    if (on_device && ((reinterpret_cast<uintptr_t>(ring) | reinterpret_cast<uintptr_t>(out)) & 15))
        api_fail(w + "device words must be 16-byte aligned");
    auto g = recorder_lock();
    // like a select: names no pool slot, flushes nothing, waits for no flight
    const RingImage *img = select_image(sel);
    Engine::get().run_lookup(img, sel->p, sel->nbits, ring, M, width, on_device, out, on_device);
    return 0;
}

// the encrypted inner products: every argument before the device is looked at, in the order the header lists the refusals
int inner_impl(const char *who, const TfheHipSelector *sel, int32_t sample, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring,
               int32_t M, int32_t width, LweSample *result, bool on_device) {
    const std::string w = std::string(who) + ": ";
    if (!ring || !result) api_fail(w + "null ring words or result");
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    selector_checked(w, sel);
    if (sample < 0 || sample >= sel->nbits) api_fail(w + "sample_index must be in 0.." + std::to_string(sel->nbits - 1));
    const Params &p = bk->bk->p;
    const int N = sel->p.N;
    if (p.N != N || p.k != sel->p.k) api_fail(w + "the selector and the cloud key belong to different rings");
    if (width < 1 || width > N || (width & (width - 1)))
        api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
    if (M < 1) api_fail(w + "M must be at least 1");
    if (on_device && (reinterpret_cast<uintptr_t>(ring) & 15)) api_fail(w + "device words must be 16-byte aligned");
    const int S = N / width, R = (int)(((int64_t)M + S - 1) / S);
    auto g = recorder_lock();
    // as the unpack: every result ours, of the key's LWE dimension, not bound to the pool of another shape
    check_runs(w, UNPACK_RESULT, ResultsView(result), M, p);
    SlotPool *pool = pool_of_key(bk);
    // a flush in flight owns the key switch's partial sums; what is recorded and has not run stays recorded
    finish_flight_locked();
    const RingImage *img = select_image(sel);     // out of device memory: ApiError, nothing has changed
    import_into_fresh_slots(pool, ResultsView(result), M, [&](const int32_t *slots) {
        Engine::get().run_inner(img, sel->p, sample, bk->bk->dev, ring, R, on_device, M, width, pool, slots, nullptr, nullptr, !on_device);
    });
    return 0;
}

// the two raw forms: the full products of R samples (u_out null), or the M extracted rows
int inner_raw_impl(const char *who, const TfheHipSelector *sel, int32_t sample, const Torus32 *ring, int32_t R, int32_t M, int32_t width,
                   Torus32 *u_out, Torus32 *prod_out) {
    const std::string w = std::string(who) + ": ";
    selector_checked(w, sel);
    if (!ring || (!u_out && !prod_out)) api_fail(w + "null argument");
    if (sample < 0 || sample >= sel->nbits) api_fail(w + "bit_index must be in 0.." + std::to_string(sel->nbits - 1));
    if (R < 1 || R > CMUX_MAX_COUNT) api_fail(w + "count must be in 1.." + std::to_string(CMUX_MAX_COUNT));
    const int N = sel->p.N;
    if (u_out) {
        if (width < 1 || width > N || (width & (width - 1))) api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
        const int64_t S = N / width;
        if (M <= (R - 1) * S || M > R * S) api_fail(w + "M must name an entry of the last of the R samples");
    }
    auto g = recorder_lock();
    finish_flight_locked();                                   // (the row buffer is the unpack's)
    const RingImage *img = select_image(sel);
    Engine::get().run_inner(img, sel->p, sample, nullptr, ring, R, false, M, u_out ? width : N, nullptr, nullptr, u_out, prod_out, true);
    return 0;
}

}  // namespace

TfheHipSelector *tfhe_hip::new_selector_object(const std::string &w, const TFheGateBootstrappingParameterSet *params, int32_t nbits) {
    if (!params || !params->in_out_params) { set_error(w + "null parameter set"); return nullptr; }
    if (nbits < 0 || nbits > SELECT_MAX_BITS) { set_error(w + "nbits must be in 0.." + std::to_string(SELECT_MAX_BITS)); return nullptr; }
    const Params &p = params_of(params);
    // what a cloud key of this set would be refused for (the CRT range, the kernel forms' gadget range), then the CMUX
    // kernel's own two bounds
    if (const char *why = unsupported_reason(p)) { set_error(w + why); return nullptr; }
    if (const char *why = cmux_gadget_error(p.N, p.k, p.l, p.Bgbit)) { set_error(w + why); return nullptr; }
    return new TfheHipSelector{SELECT_MAGIC, p, nbits, std::vector<Torus32>(), nullptr, std::vector<uint32_t>(), std::vector<Torus32>(), 0};
}
bool tfhe_hip::selector_ok(const TfheHipSelector *sel) { return sel && sel->magic == SELECT_MAGIC; }
const TfheHipSelector *tfhe_hip::selector_checked(const std::string &w, const TfheHipSelector *sel) {
    if (!sel || sel->magic != SELECT_MAGIC) api_fail(w + "null or deleted selector");
    return sel;
}

// the selector's image, made at first use (under the recorder lock); null for a selector of no bits
const RingImage *tfhe_hip::select_image(const TfheHipSelector *csel) {
    auto *sel = const_cast<TfheHipSelector *>(csel);
    if (sel->img || sel->nbits < 1) return sel->img;
    const int64_t body_bytes = (int64_t)sel->nbits * sel->p.kpl() * sel->p.N * 4;
    if (sel->mask_seed.empty()) {
        sel->img = Engine::get().upload_selector(sel->p, sel->words.data(), sel->nbits);
        sel->upload_bytes = body_bytes * (sel->p.k + 1);
    } else {
        // a compressed selector: the bodies go up, the masks are written on the card (expand.hip)
        sel->img = Engine::get().upload_selector_seeded(sel->p, sel->mask_seed.data(), sel->body.data(), sel->nbits);
        sel->upload_bytes = body_bytes;
    }
    return sel->img;
}

extern "C" {

int64_t tfhe_hip_tgsw_words(const TFheGateBootstrappingParameterSet *params) {
    if (!params || !params->in_out_params) { set_error("tfhe_hip_tgsw_words: null parameter set"); return -1; }
    const Params &p = params_of(params);
    return (int64_t)p.kpl() * (p.k + 1) * p.N;
}

int tfhe_hip_tgsw_encrypt_bits(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                               Torus32 *out_words) {
    return tgsw_encrypt_impl("tfhe_hip_tgsw_encrypt_bits", secret, bits, count, out_words, nullptr);
}
int tfhe_hip_tgsw_encrypt_bits_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                      Torus32 *out_words, uint64_t seed) {
    return tgsw_encrypt_impl("tfhe_hip_tgsw_encrypt_bits_seeded", secret, bits, count, out_words, &seed);
}

int tfhe_hip_tgsw_encrypt_polys(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                Torus32 *out_words) {
    return tgsw_encrypt_impl("tfhe_hip_tgsw_encrypt_polys", secret, polys, count, out_words, nullptr, true);
}
int tfhe_hip_tgsw_encrypt_polys_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                       Torus32 *out_words, uint64_t seed) {
    return tgsw_encrypt_impl("tfhe_hip_tgsw_encrypt_polys_seeded", secret, polys, count, out_words, &seed, true);
}

int tfhe_hip_ring_center_words(const TFheGateBootstrappingParameterSet *params, Torus32 *words, int64_t count) {
    const std::string w = "tfhe_hip_ring_center_words: ";
    if (!params || !params->in_out_params || !words) { set_error(w + "null argument"); return -1; }
    if (count < 0) { set_error(w + "count must not be negative"); return -1; }
    const Params &p = params_of(params);
    const int low = 32 - p.l * p.Bgbit;                    // the bits the decomposition drops
    if (low <= 0) return 0;
    const uint32_t half = 1u << (low - 1);
    for (int64_t j = 0; j < count; ++j) words[j] = (Torus32)((uint32_t)words[j] + half);
    return 0;
}

TfheHipSelector *tfhe_hip_new_selector(const TFheGateBootstrappingParameterSet *params, const Torus32 *words, int32_t nbits) {
    const std::string w = "tfhe_hip_new_selector: ";
    // every argument before the device is looked at: a refusal has no effect
    if (!params || !params->in_out_params) { set_error(w + "null parameter set"); return nullptr; }
    if (nbits < 0 || nbits > SELECT_MAX_BITS) { set_error(w + "nbits must be in 0.." + std::to_string(SELECT_MAX_BITS)); return nullptr; }
    if (nbits > 0 && !words) { set_error(w + "null words"); return nullptr; }
    TfheHipSelector *sel = new_selector_object(w, params, nbits);
    if (sel && nbits > 0) sel->words.assign(words, words + (size_t)nbits * sel->p.kpl() * (sel->p.k + 1) * sel->p.N);
    return sel;
}
void tfhe_hip_delete_selector(TfheHipSelector *sel) {
    if (!sel) return;
    if (sel->magic != SELECT_MAGIC) { set_error("tfhe_hip_delete_selector: not a selector (or already deleted)"); return; }
    auto g = recorder_lock();
    Engine::get().free_selector(sel->img);                // (waits for the stream: a select in flight reads the image)
    sel->magic = 0;
    delete sel;
}
int32_t tfhe_hip_selector_bits(const TfheHipSelector *sel) {
    if (!sel || sel->magic != SELECT_MAGIC) { set_error("tfhe_hip_selector_bits: null or deleted selector"); return -1; }
    return sel->nbits;
}

int tfhe_hip_ring_select(const TfheHipSelector *sel, const Torus32 *ring_words, int32_t M, Torus32 *out_ring_words) {
    return guarded_rc([&] { return select_impl("tfhe_hip_ring_select", sel, ring_words, M, out_ring_words, false); });
}
int tfhe_hip_ring_select_device(const TfheHipSelector *sel, const void *device_ring_words, int32_t M, void *device_out) {
    return guarded_rc([&] {
        return select_impl("tfhe_hip_ring_select_device", sel, static_cast<const Torus32 *>(device_ring_words), M,
                           static_cast<Torus32 *>(device_out), true);
    });
}

int tfhe_hip_ring_lookup(const TfheHipSelector *sel, const Torus32 *ring_words, int32_t M, int32_t width, Torus32 *out_ring_words) {
    return guarded_rc([&] { return lookup_impl("tfhe_hip_ring_lookup", sel, ring_words, M, width, out_ring_words, false); });
}
int tfhe_hip_ring_lookup_device(const TfheHipSelector *sel, const void *device_ring_words, int32_t M, int32_t width, void *device_out) {
    return guarded_rc([&] {
        return lookup_impl("tfhe_hip_ring_lookup_device", sel, static_cast<const Torus32 *>(device_ring_words), M, width,
                           static_cast<Torus32 *>(device_out), true);
    });
}

int tfhe_hip_kernel_ring_cmux_rotate(const TfheHipSelector *sel, int32_t bit_index, int32_t rot, const Torus32 *d0_words, int32_t count,
                                     Torus32 *out_words) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_ring_cmux_rotate: ";
        selector_checked(w, sel);
        if (!d0_words || !out_words) api_fail(w + "null argument");
        if (bit_index < 0 || bit_index >= sel->nbits) api_fail(w + "bit_index must be in 0.." + std::to_string(sel->nbits - 1));
        if (rot < 1 || rot >= sel->p.N) api_fail(w + "rot must be in 1.." + std::to_string(sel->p.N - 1));
        if (count < 1 || count > CMUX_MAX_COUNT) api_fail(w + "count must be in 1.." + std::to_string(CMUX_MAX_COUNT));
        auto g = recorder_lock();
        const RingImage *img = select_image(sel);
        Engine::get().run_cmux(img, sel->p, bit_index, nullptr, d0_words, count, out_words, rot);
        return 0;
    });
}

int tfhe_hip_kernel_ring_cmux(const TfheHipSelector *sel, int32_t bit_index, const Torus32 *d1_words, const Torus32 *d0_words,
                              int32_t count, Torus32 *out_words) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_ring_cmux: ";
        selector_checked(w, sel);
        if (!d1_words || !d0_words || !out_words) api_fail(w + "null argument");
        if (bit_index < 0 || bit_index >= sel->nbits) api_fail(w + "bit_index must be in 0.." + std::to_string(sel->nbits - 1));
        if (count < 1 || count > CMUX_MAX_COUNT) api_fail(w + "count must be in 1.." + std::to_string(CMUX_MAX_COUNT));
        auto g = recorder_lock();
        const RingImage *img = select_image(sel);
        Engine::get().run_cmux(img, sel->p, bit_index, d1_words, d0_words, count, out_words);
        return 0;
    });
}

int tfhe_hip_ring_inner(const TfheHipSelector *sel, int32_t sample_index, const TFheGateBootstrappingCloudKeySet *bk,
                        const Torus32 *ring_words, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] { return inner_impl("tfhe_hip_ring_inner", sel, sample_index, bk, ring_words, M, width, result, false); });
}
int tfhe_hip_ring_inner_device(const TfheHipSelector *sel, int32_t sample_index, const TFheGateBootstrappingCloudKeySet *bk,
                               const void *device_ring_words, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] {
        return inner_impl("tfhe_hip_ring_inner_device", sel, sample_index, bk, static_cast<const Torus32 *>(device_ring_words), M, width,
                          result, true);
    });
}

int tfhe_hip_kernel_ring_product(const TfheHipSelector *sel, int32_t bit_index, const Torus32 *ring_words, int32_t count,
                                 Torus32 *out_words) {
    return guarded_rc([&] { return inner_raw_impl("tfhe_hip_kernel_ring_product", sel, bit_index, ring_words, count, 0, 0, nullptr, out_words); });
}
int tfhe_hip_kernel_ring_inner_rows(const TfheHipSelector *sel, int32_t bit_index, const Torus32 *ring_words, int32_t R, int32_t M,
                                    int32_t width, Torus32 *out_rows) {
    return guarded_rc([&] { return inner_raw_impl("tfhe_hip_kernel_ring_inner_rows", sel, bit_index, ring_words, R, M, width, out_rows, nullptr); });
}

double tfhe_hip_last_select_ms(void) {
    auto g = recorder_lock();
    return Engine::get().last_select_ms();
}

int tfhe_hip_test_select_bounds(int32_t N, int32_t l, int32_t Bgbit) {
    if ((N != 1024 && N != 2048) || l < 1 || Bgbit < 1 || Bgbit > CMUX_MAX_BGBIT || l * Bgbit > 32) {
        set_error("test_select_bounds: bad arguments");
        return -1;
    }
    return (cmux_mac_ok(N, 2 * l) ? 0 : 1) | (cmux_crt_ok(N, 2 * l, Bgbit) ? 0 : 2);
}

}  // extern "C"
