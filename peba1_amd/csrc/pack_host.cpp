// pack_host.cpp -- host side of the packing key switch: the key object, key generation, decryption of a packed
// sample and the C ABI (include/tfhe_hip.h "packing key switch").  No arithmetic of the pack itself happens here
// (pack.hip); key generation and decryption run on the CPU like those of the LWE samples.
#include <cstring>
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

namespace {
constexpr uint32_t PACK_MAGIC = 0x5041434Bu;
}  // namespace

// ---- what the other host files use (shim_internal.hpp) ----
void tfhe_hip::pack_add_mul_by_bits(uint32_t *body, const uint32_t *mask, const int32_t *bits, int N, uint32_t sign) {
    for (int i = 0; i < N; ++i) {
        if (!bits[i]) continue;
        for (int j = 0; j < N - i; ++j) body[i + j] += sign * mask[j];
        for (int j = N - i; j < N; ++j) body[i + j - N] -= sign * mask[j];
    }
}

TfheHipPackingKey *tfhe_hip::new_packing_key_object(const char *who, const Params &p, int32_t pk_t, int32_t pk_basebit, bool with_rows) {
    if (pk_t == 0 && pk_basebit == 0) { pk_t = p.ks_t; pk_basebit = p.ks_basebit; }
    if (const char *why = pack_decomp_error(p.N, p.k, pk_t, pk_basebit)) { set_error(std::string(who) + ": " + why); return nullptr; }
    if (p.n < 1 || p.n > 1024) { set_error(std::string(who) + ": LWE dimension n must be in [1, 1024]"); return nullptr; }
    auto *key = new TfheHipPackingKey{PACK_MAGIC, p, pk_t, pk_basebit, std::vector<Torus32>(), {}};
    if (with_rows) key->rows.assign((size_t)p.n * pk_t * (p.k + 1) * p.N, 0);
    return key;
}

bool tfhe_hip::pack_same_set(const Params &a, const Params &b) {
    return a.n == b.n && a.N == b.N && a.k == b.k && a.l == b.l && a.Bgbit == b.Bgbit && a.ks_t == b.ks_t &&
           a.ks_basebit == b.ks_basebit;
}

const TfheHipPackingKey *tfhe_hip::pack_key_checked(const char *who, const TfheHipPackingKey *key) {
    if (!key || key->magic != PACK_MAGIC) api_fail(std::string(who) + ": null or deleted packing key");
    return key;
}

const uint32_t *tfhe_hip::pack_image(const TfheHipPackingKey *ckey, const TFheGateBootstrappingCloudKeySet *bk) {
    auto *key = const_cast<TfheHipPackingKey *>(ckey);
    if (key->img.empty())
        key->img = key->mask_seed.empty()
                       ? Engine::get().upload_pack_image(bk->bk->dev, key->rows.data(), key->t)
                       : Engine::get().expand_pack_image(bk->bk->dev, key->mask_seed.data(), key->body.data(), key->t);
    return key->img.get();
}

void tfhe_hip::expand_packing_rows_host(const Params &p, int t, const uint32_t seed10[10], const Torus32 *body, std::vector<Torus32> &rows) {
    const size_t N = (size_t)p.N, nrows = (size_t)p.n * t;
    Rng mask = Rng::keyed(seed10);
    rows.assign(nrows * 2 * N, 0);
    for (size_t r = 0; r < nrows; ++r) {
        Torus32 *smp = rows.data() + r * 2 * N;
        for (size_t j = 0; j < N; ++j) smp[j] = mask.torus();
        std::memcpy(smp + N, body + r * N, N * sizeof(Torus32));
    }
}

namespace {

// The draw order (include/tfhe_hip.h): for i < n, for p < t: the kN mask words, then the N noise samples.
void fill_packing_key(TfheHipPackingKey &key, const TfheHipSecretKey &sk, Rng &secret, Rng &mask) {
    const Params &p = key.p;
    const int N = p.N, k = p.k;
    for (int i = 0; i < p.n; ++i)
        for (int d = 0; d < key.t; ++d) {
            uint32_t *smp = reinterpret_cast<uint32_t *>(key.rows.data()) + ((size_t)i * key.t + d) * (size_t)(k + 1) * N;
            uint32_t *body = smp + (size_t)k * N;
            for (int u = 0; u < k; ++u)
                for (int j = 0; j < N; ++j) smp[(size_t)u * N + j] = (uint32_t)mask.torus();
            for (int j = 0; j < N; ++j) body[j] = (uint32_t)dtot32(secret.gauss(p.bk_stdev));
            for (int u = 0; u < k; ++u) pack_add_mul_by_bits(body, smp + (size_t)u * N, sk.tlwe_key.data() + (size_t)u * N, N, 1u);
            body[0] += (uint32_t)sk.lwe_key[i] << (32 - (d + 1) * key.basebit);
        }
}

TfheHipPackingKey *make_packing_key(const char *who, const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t,
                                    int32_t pk_basebit, const uint64_t *seed) {
    if (!secret || !secret->lwe_key) { set_error(std::string(who) + ": null secret keyset"); return nullptr; }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    TfheHipPackingKey *key = new_packing_key_object(who, sk.p, pk_t, pk_basebit);
    if (!key) return nullptr;
    if (seed) {
        Rng both(*seed);                                  // a stream of its own: the keyset's streams are long gone
        fill_packing_key(*key, sk, both, both);
    } else {
        Rng noise = Rng::secure(), mask = Rng::secure();  // two fresh ChaCha20 streams, as for a keyset
        fill_packing_key(*key, sk, noise, mask);
    }
    return key;
}

int pack_impl(const TfheHipPackingKey *key, const LweSample *samples, int32_t count, const TFheGateBootstrappingCloudKeySet *bk,
              Torus32 *out, bool device_dst) {
    const char *who = "tfhe_hip_pack_samples";
    pack_key_checked(who, key);
    if (!samples || !out) api_fail(std::string(who) + ": null samples or destination");
    if (!bk || !bk->bk) api_fail(std::string(who) + ": null cloud key");
    const Params &p = key->p;
    if (count < 1 || count > p.N) api_fail(std::string(who) + ": count must be in 1.." + std::to_string(p.N));
    if (!pack_same_set(p, bk->bk->p)) api_fail(std::string(who) + ": the cloud key belongs to another parameter set than the packing key");
    auto g = recorder_lock();
    check_runs(std::string(who) + ": ", PACK_SAMPLES, [&](int32_t) { return samples; }, 1, count, p);
    SlotPool *pool = pool_of_key(bk);
    const uint32_t *img = pack_image(key, bk);            // out of device memory: ApiError, nothing has changed
    // an observation point like the exports: what is recorded runs first (the device form only enqueues it)
    flush_pending_locked(!device_dst);
    std::vector<int32_t> slots(count);
    for (int32_t i = 0; i < count; ++i) slots[i] = ensure_slot(&samples[i], pool);
    Engine::get().run_pack(bk->bk->dev, img, key->t, key->basebit, pool, slots.data(), nullptr, count, 0, out, device_dst, !device_dst);
    return 0;
}

// phases of all N coefficients: B - sum_u A_u S_u
void packed_phases(const TfheHipSecretKey &sk, const Torus32 *words, uint32_t *ph) {
    const int N = sk.p.N, k = sk.p.k;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(words);
    std::memcpy(ph, w + (size_t)k * N, (size_t)N * 4);
    for (int u = 0; u < k; ++u) pack_add_mul_by_bits(ph, w + (size_t)u * N, sk.tlwe_key.data() + (size_t)u * N, N, 0u - 1u);
}

}  // namespace

extern "C" {

TfheHipPackingKey *tfhe_hip_new_packing_key(const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t, int32_t pk_basebit) {
    return make_packing_key("tfhe_hip_new_packing_key", secret, pk_t, pk_basebit, nullptr);
}
TfheHipPackingKey *tfhe_hip_new_packing_key_seeded(const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t, int32_t pk_basebit,
                                                   uint64_t seed) {
    return make_packing_key("tfhe_hip_new_packing_key_seeded", secret, pk_t, pk_basebit, &seed);
}
TfheHipPackingKey *tfhe_hip_new_packing_key_from_words(const TFheGateBootstrappingParameterSet *params, int32_t pk_t,
                                                       int32_t pk_basebit, const Torus32 *words) {
    const char *who = "tfhe_hip_new_packing_key_from_words";
    if (!params || !params->in_out_params || !words) { set_error(std::string(who) + ": null parameter set or words"); return nullptr; }
    TfheHipPackingKey *key = new_packing_key_object(who, params_of(params), pk_t, pk_basebit);
    if (key) std::memcpy(key->rows.data(), words, key->rows.size() * 4);
    return key;
}
void tfhe_hip_delete_packing_key(TfheHipPackingKey *key) {
    if (!key) return;
    if (key->magic != PACK_MAGIC) { set_error("tfhe_hip_delete_packing_key: not a packing key (or already deleted)"); return; }
    auto g = recorder_lock();
    Engine::get().free_pack_image(key->img);      // (waits for the stream: a pack in flight reads the image)
    key->magic = 0;
    delete key;
}
const Torus32 *tfhe_hip_packing_key_words(const TfheHipPackingKey *key, int64_t *count) {
    if (!key || key->magic != PACK_MAGIC) { set_error("tfhe_hip_packing_key_words: null or deleted packing key"); if (count) *count = 0; return nullptr; }
    if (!key->mask_seed.empty() && key->rows.empty()) {   // a device-expanded key: the host rows are made when asked for
        auto g = recorder_lock();
        auto *k = const_cast<TfheHipPackingKey *>(key);
        if (k->rows.empty()) expand_packing_rows_host(k->p, k->t, k->mask_seed.data(), k->body.data(), k->rows);
    }
    if (count) *count = (int64_t)key->rows.size();
    return key->rows.data();
}
int tfhe_hip_packing_key_decomposition(const TfheHipPackingKey *key, int32_t *pk_t, int32_t *pk_basebit) {
    if (!key || key->magic != PACK_MAGIC) { set_error("tfhe_hip_packing_key_decomposition: null or deleted packing key"); return -1; }
    if (pk_t) *pk_t = key->t;
    if (pk_basebit) *pk_basebit = key->basebit;
    return 0;
}

int tfhe_hip_pack_samples(const TfheHipPackingKey *key, const LweSample *samples, int32_t count,
                          const TFheGateBootstrappingCloudKeySet *bk, Torus32 *out_words) {
    return guarded_rc([&] { return pack_impl(key, samples, count, bk, out_words, false); });
}
int tfhe_hip_pack_samples_device(const TfheHipPackingKey *key, const LweSample *samples, int32_t count,
                                 const TFheGateBootstrappingCloudKeySet *bk, void *device_words) {
    return guarded_rc([&] { return pack_impl(key, samples, count, bk, static_cast<Torus32 *>(device_words), true); });
}

int tfhe_hip_packed_phase(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *words, Torus32 *out_phases) {
    if (!secret || !secret->lwe_key || !words || !out_phases) { set_error("tfhe_hip_packed_phase: null argument"); return -1; }
    packed_phases(*secret->lwe_key, words, reinterpret_cast<uint32_t *>(out_phases));
    return 0;
}
int tfhe_hip_packed_decrypt_bits(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *words, int32_t count,
                                 int32_t *out_bits) {
    if (!secret || !secret->lwe_key || !words || !out_bits) { set_error("tfhe_hip_packed_decrypt_bits: null argument"); return -1; }
    const int N = secret->lwe_key->p.N;
    if (count < 1 || count > N) { set_error("tfhe_hip_packed_decrypt_bits: count must be in 1.." + std::to_string(N)); return -1; }
    std::vector<uint32_t> ph((size_t)N);
    packed_phases(*secret->lwe_key, words, ph.data());
    for (int32_t j = 0; j < count; ++j) out_bits[j] = (int32_t)ph[(size_t)j] > 0 ? 1 : 0;
    return 0;
}

int tfhe_hip_test_pack_bounds(int32_t N, int32_t rows, int32_t basebit) {
    if ((N != 1024 && N != 2048) || rows < 1 || rows > (1 << 20) || basebit < 1 || basebit > PACK_MAX_BASEBIT) {
        set_error("test_pack_bounds: bad arguments");
        return -1;
    }
    return (pack_mac_ok(N, rows) ? 0 : 1) | (pack_crt_ok(N, rows, basebit) ? 0 : 2);
}

int tfhe_hip_kernel_pack(const TfheHipPackingKey *key, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *sample_words,
                         int32_t count, int32_t idx_per_wg, Torus32 *out_words) {
    return guarded_rc([&] {
        const char *who = "tfhe_hip_kernel_pack";
        pack_key_checked(who, key);
        if (!bk || !bk->bk || !sample_words || !out_words) api_fail(std::string(who) + ": null argument");
        if (count < 1 || count > key->p.N || idx_per_wg < 0) api_fail(std::string(who) + ": count must be in 1..N and idx_per_wg >= 0");
        if (!pack_same_set(key->p, bk->bk->p)) api_fail(std::string(who) + ": the cloud key belongs to another parameter set than the packing key");
        auto g = recorder_lock();
        pool_of_key(bk);
        const uint32_t *img = pack_image(key, bk);
        Engine::get().wait_flight();
        Engine::get().run_pack(bk->bk->dev, img, key->t, key->basebit, nullptr, nullptr, sample_words, count, idx_per_wg, out_words, false, true);
        return 0;
    });
}

}  // extern "C"
