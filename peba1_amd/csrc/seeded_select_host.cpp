// seeded_select_host.cpp -- host side of the seed-compressed selectors and TGSW probes (include/tfhe_hip.h "seed-compressed
// selectors"): the compressed encryptors of bits and polynomials, the host expansion, the compressed selector and the
// upload-bytes getter.  The selector object, its first-use image and every entry that takes a selector are
// select_host.cpp's; the negacyclic product is pack_host.cpp's; the device side is Engine::upload_selector_seeded, which
// runs expand.hip's launch_expand_bk at rows = nbits (k+1) l.  An object of its own in build.sh: shim.cpp's list of included
// files is closed (tests/test_host_sources_cpu.py).
#include <cstring>
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

static_assert(TFHE_HIP_TGSW_COMPRESSED_WORDS(1, 3, 1024, 1) == 6154, "the header's count for one bit at P128");

namespace {

// The record of `count` samples: the seed, then for every sample, for every row (u, p) in word order, the body of the row
// whose k mask polynomials are the next k N stream words of `seed`.  The gadget term g_p m of the row cannot sit on a mask
// polynomial (the masks are the stream words verbatim), so it goes on the body: + g_p m for u = k, - g_p (m s_u) for u < k --
// the phase b - sum a s of tgsw_encrypt_into's row, as generate_compressed_key does for the bootstrapping key.
// polys false: sample b encrypts the bit msg[b] (a constant polynomial); true: the polynomial at msg[b N .. + N).
// noise: N gaussians of bk_stdev per row, in row order.
void tgsw_compressed_into(const TfheHipSecretKey &sk, const int32_t *msg, bool polys, int32_t count, const uint32_t seed[10],
                          Rng &noise, uint32_t *out) {
    const Params &p = sk.p;
    const int N = p.N, k = p.k, l = p.l, kpl = p.kpl();
    Rng mask = Rng::keyed(seed);
    std::memcpy(out, seed, 10 * sizeof(uint32_t));
    std::vector<uint32_t> m((size_t)k * N), gm((size_t)N);
    for (int32_t b = 0; b < count; ++b)
        for (int row = 0; row < kpl; ++row) {
            uint32_t *body = out + 10 + ((size_t)b * kpl + row) * N;
            for (auto &w : m) w = (uint32_t)mask.torus();
            for (int j = 0; j < N; ++j) body[j] = (uint32_t)dtot32(noise.gauss(p.bk_stdev));
            for (int u = 0; u < k; ++u) pack_add_mul_by_bits(body, m.data() + (size_t)u * N, sk.tlwe_key.data() + (size_t)u * N, N, 1u);
            const int u = row / l, pp = row % l;
            const int shift = 32 - (pp + 1) * p.Bgbit;
            for (int j = 0; j < N; ++j)
                gm[j] = polys ? (uint32_t)msg[(size_t)b * N + j] << shift : j ? 0u : (uint32_t)(msg[b] ? 1 : 0) << shift;
            if (u == k)
                for (int j = 0; j < N; ++j) body[j] += gm[j];
            else pack_add_mul_by_bits(body, gm.data(), sk.tlwe_key.data() + (size_t)u * N, N, 0u - 1u);
        }
}

// seed null: ten fresh seed words and a fresh noise stream from the OS; else ONE seeded generator for this record alone,
// whose first ten `torus` draws are the seed words and whose later draws are the noise
int tgsw_compressed_impl(const char *who, const TFheGateBootstrappingSecretKeySet *secret, const int32_t *msg, int32_t count,
                         Torus32 *out, const uint64_t *seed, bool polys) {
    if (!secret || !secret->lwe_key || !msg || !out) { set_error(std::string(who) + ": null argument"); return -1; }
    if (count < 1 || count > SELECT_MAX_BITS) {
        set_error(std::string(who) + ": count must be in 1.." + std::to_string(SELECT_MAX_BITS));
        return -1;
    }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    uint32_t seed10[10];
    if (seed) {
        Rng both(*seed);
        for (auto &w : seed10) w = (uint32_t)both.torus();
        tgsw_compressed_into(sk, msg, polys, count, seed10, both, reinterpret_cast<uint32_t *>(out));
    } else {
        os_seed(seed10);                                      // ONE SEED PER RECORD: fresh for every call
        Rng noise = Rng::secure();
        tgsw_compressed_into(sk, msg, polys, count, seed10, noise, reinterpret_cast<uint32_t *>(out));
    }
    return 0;
}

}  // namespace

extern "C" {

int64_t tfhe_hip_tgsw_compressed_words(const TFheGateBootstrappingParameterSet *params, int32_t count) {
    if (!params || !params->in_out_params) { set_error("tfhe_hip_tgsw_compressed_words: null parameter set"); return -1; }
    if (count < 0) { set_error("tfhe_hip_tgsw_compressed_words: count must not be negative"); return -1; }
    const Params &p = params_of(params);
    return TFHE_HIP_TGSW_COMPRESSED_WORDS(p.k, p.l, p.N, count);
}

int tfhe_hip_tgsw_encrypt_bits_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                          Torus32 *out_words) {
    return tgsw_compressed_impl("tfhe_hip_tgsw_encrypt_bits_compressed", secret, bits, count, out_words, nullptr, false);
}
int tfhe_hip_tgsw_encrypt_bits_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                                 Torus32 *out_words, uint64_t seed) {
    return tgsw_compressed_impl("tfhe_hip_tgsw_encrypt_bits_compressed_seeded", secret, bits, count, out_words, &seed, false);
}
int tfhe_hip_tgsw_encrypt_polys_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                           Torus32 *out_words) {
    return tgsw_compressed_impl("tfhe_hip_tgsw_encrypt_polys_compressed", secret, polys, count, out_words, nullptr, true);
}
int tfhe_hip_tgsw_encrypt_polys_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *polys, int32_t count,
                                                  Torus32 *out_words, uint64_t seed) {
    return tgsw_compressed_impl("tfhe_hip_tgsw_encrypt_polys_compressed_seeded", secret, polys, count, out_words, &seed, true);
}

int tfhe_hip_tgsw_expand_host(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words, int32_t count,
                              Torus32 *out_words) {
    const std::string w = "tfhe_hip_tgsw_expand_host: ";
    if (!params || !params->in_out_params || !compressed_words || !out_words) { set_error(w + "null argument"); return -1; }
    if (count < 1 || count > SELECT_MAX_BITS) { set_error(w + "count must be in 1.." + std::to_string(SELECT_MAX_BITS)); return -1; }
    const Params &p = params_of(params);
    const size_t rows = (size_t)count * p.kpl(), kN = (size_t)p.k * p.N;
    // masks from ONE sequential stream, as expand_masks_host draws a cloud key's
    Rng mask = Rng::keyed(reinterpret_cast<const uint32_t *>(compressed_words));
    for (size_t r = 0; r < rows; ++r) {
        Torus32 *smp = out_words + r * (kN + p.N);
        for (size_t j = 0; j < kN; ++j) smp[j] = mask.torus();
        std::memcpy(smp + kN, compressed_words + 10 + r * p.N, (size_t)p.N * sizeof(Torus32));
    }
    return 0;
}

TfheHipSelector *tfhe_hip_new_selector_compressed(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words,
                                                  int32_t count, int32_t nbits) {
    const std::string w = "tfhe_hip_new_selector_compressed: ";
    // every argument before the device is looked at: a refusal has no effect
    if (!params || !params->in_out_params) { set_error(w + "null parameter set"); return nullptr; }
    if (!compressed_words) { set_error(w + "null words"); return nullptr; }
    if (count < 1 || count > SELECT_MAX_BITS) { set_error(w + "count must be in 1.." + std::to_string(SELECT_MAX_BITS)); return nullptr; }
    if (nbits >= 0 && nbits <= SELECT_MAX_BITS && nbits > count) {
        set_error(w + "nbits = " + std::to_string(nbits) + " is above the " + std::to_string(count) + " samples of the record");
        return nullptr;
    }
    TfheHipSelector *sel = new_selector_object(w, params, nbits);
    if (!sel) return nullptr;
    // the first nbits samples of the record: their masks are the first nbits (k+1) l k N words of the record's stream
    const uint32_t *seed = reinterpret_cast<const uint32_t *>(compressed_words);
    sel->mask_seed.assign(seed, seed + 10);
    sel->body.assign(compressed_words + 10, compressed_words + 10 + (size_t)nbits * sel->p.kpl() * sel->p.N);
    return sel;
}

int64_t tfhe_hip_selector_upload_bytes(const TfheHipSelector *sel) {
    if (!selector_ok(sel)) { set_error("tfhe_hip_selector_upload_bytes: null or deleted selector"); return -1; }
    auto g = recorder_lock();                                 // (the image is made under it)
    return sel->upload_bytes;
}

}  // extern "C"
