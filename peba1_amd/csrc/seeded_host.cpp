// seeded_host.cpp -- host side of the seed-compressed packing keys and ring samples: the compressed key object, its
// generators, the two expansions, compressed ring encryption and the C ABI of the seeded unpack (include/tfhe_hip.h
// "seed-compressed packing keys and ring samples").  The packing key, the negacyclic product and the unpack are those of
// pack_host.cpp and unpack_host.cpp.  The device side is Engine::expand_pack_image (expand.hip) and the seeded extract
// kernel (unpack.hip); the file form is in io.cpp.
#include <cstring>
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

namespace {

TfheHipCompressedPackingKey *new_compressed_pack_object(const char *who, const Params &p, int32_t pk_t, int32_t pk_basebit) {
    if (pk_t == 0 && pk_basebit == 0) { pk_t = p.ks_t; pk_basebit = p.ks_basebit; }
    if (const char *why = pack_decomp_error(p.N, p.k, pk_t, pk_basebit)) { set_error(std::string(who) + ": " + why); return nullptr; }
    if (p.n < 1 || p.n > 1024) { set_error(std::string(who) + ": LWE dimension n must be in [1, 1024]"); return nullptr; }
    auto *key = new TfheHipCompressedPackingKey();
    key->magic = COMPRESSED_PACK_MAGIC;
    key->p = p;
    key->t = pk_t;
    key->basebit = pk_basebit;
    return key;
}

// body = mask * S + e + mu of one ring sample whose N mask words are the next N draws of `mask` (k = 1); mu may be null
void seeded_ring_body(const TfheHipSecretKey &sk, Rng &mask, Rng &noise, const Torus32 *mu, uint32_t *body) {
    const int N = sk.p.N;
    std::vector<uint32_t> m((size_t)N);
    for (auto &w : m) w = (uint32_t)mask.torus();
    for (int j = 0; j < N; ++j) body[j] = (uint32_t)dtot32(noise.gauss(sk.p.bk_stdev)) + (mu ? (uint32_t)mu[j] : 0u);
    pack_add_mul_by_bits(body, m.data(), sk.tlwe_key.data(), N, 1u);
}

// rows in [i][p] order: the N mask words of a row from the key's stream, then its N noise samples from `noise`
void fill_compressed_packing_key(TfheHipCompressedPackingKey &key, const TfheHipSecretKey &sk, Rng &noise) {
    const Params &p = key.p;
    Rng mask = Rng::keyed(key.seed);
    key.body.assign((size_t)p.n * key.t * p.N, 0);
    for (int i = 0; i < p.n; ++i)
        for (int d = 0; d < key.t; ++d) {
            uint32_t *body = reinterpret_cast<uint32_t *>(key.body.data()) + ((size_t)i * key.t + d) * p.N;
            seeded_ring_body(sk, mask, noise, nullptr, body);
            body[0] += (uint32_t)sk.lwe_key[i] << (32 - (d + 1) * key.basebit);
        }
}

TfheHipCompressedPackingKey *make_compressed_packing_key(const char *who, const TFheGateBootstrappingSecretKeySet *secret,
                                                         int32_t pk_t, int32_t pk_basebit, const uint64_t *noise_seed,
                                                         const uint32_t *mask_seed10) {
    if (!secret || !secret->lwe_key) { set_error(std::string(who) + ": null secret keyset"); return nullptr; }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    TfheHipCompressedPackingKey *key = new_compressed_pack_object(who, sk.p, pk_t, pk_basebit);
    if (!key) return nullptr;
    if (noise_seed) {
        std::memcpy(key->seed, mask_seed10, sizeof key->seed);
        Rng noise(*noise_seed);
        fill_compressed_packing_key(*key, sk, noise);
    } else {
        os_seed(key->seed);
        Rng noise = Rng::secure();
        fill_compressed_packing_key(*key, sk, noise);
    }
    return key;
}

bool compressed_pack_ok(const char *who, const TfheHipCompressedPackingKey *key) {
    if (key && key->magic == COMPRESSED_PACK_MAGIC) return true;
    set_error(std::string(who) + ": null or deleted compressed packing key");
    return false;
}

// mask_seed10 null: a fresh seed from the OS and fresh noise; else the fixture form
int ring_encrypt_compressed_impl(const char *who, const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu,
                                 const int32_t *bits, int32_t count, Torus32 *out, const uint32_t *mask_seed10, uint64_t noise_seed,
                                 bool fixture) {
    if (!secret || !secret->lwe_key || (!mu && !bits) || !out || (fixture && !mask_seed10)) { set_error(std::string(who) + ": null argument"); return -1; }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    const int N = sk.p.N;
    if (sk.p.k != 1) { set_error(std::string(who) + ": compressed ring samples are defined for k = 1"); return -1; }
    std::vector<Torus32> msg;
    if (bits) {
        if (!ring_message_of_bits(who, bits, count, N, msg)) return -1;
        mu = msg.data();
    }
    uint32_t *w = reinterpret_cast<uint32_t *>(out);
    uint32_t seed[10];
    if (fixture) std::memcpy(seed, mask_seed10, sizeof seed);
    else os_seed(seed);
    Rng mask = Rng::keyed(seed);
    Rng noise = fixture ? Rng(noise_seed) : Rng::secure();
    std::vector<uint32_t> body((size_t)N);                 // (mu may alias out)
    seeded_ring_body(sk, mask, noise, mu, body.data());
    std::memcpy(w, seed, sizeof seed);
    std::memcpy(w + 10, body.data(), (size_t)N * 4);
    return 0;
}

}  // namespace

extern "C" {

TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key(const TFheGateBootstrappingSecretKeySet *secret, int32_t pk_t,
                                                                 int32_t pk_basebit) {
    return make_compressed_packing_key("tfhe_hip_new_compressed_packing_key", secret, pk_t, pk_basebit, nullptr, nullptr);
}
TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key_seeded(const TFheGateBootstrappingSecretKeySet *secret,
                                                                        int32_t pk_t, int32_t pk_basebit, uint64_t noise_seed,
                                                                        const uint32_t *mask_seed10) {
    const char *who = "tfhe_hip_new_compressed_packing_key_seeded";
    if (!mask_seed10) { set_error(std::string(who) + ": null mask seed"); return nullptr; }
    return make_compressed_packing_key(who, secret, pk_t, pk_basebit, &noise_seed, mask_seed10);
}
TfheHipCompressedPackingKey *tfhe_hip_new_compressed_packing_key_from_words(const TFheGateBootstrappingParameterSet *params,
                                                                            int32_t pk_t, int32_t pk_basebit,
                                                                            const uint32_t *mask_seed10, const Torus32 *body) {
    const char *who = "tfhe_hip_new_compressed_packing_key_from_words";
    if (!params || !params->in_out_params || !mask_seed10 || !body) { set_error(std::string(who) + ": null argument"); return nullptr; }
    TfheHipCompressedPackingKey *key = new_compressed_pack_object(who, params_of(params), pk_t, pk_basebit);
    if (!key) return nullptr;
    std::memcpy(key->seed, mask_seed10, sizeof key->seed);
    key->body.assign(body, body + (size_t)key->p.n * key->t * key->p.N);
    return key;
}
void tfhe_hip_delete_compressed_packing_key(TfheHipCompressedPackingKey *key) {
    if (!key) return;
    if (key->magic != COMPRESSED_PACK_MAGIC) { set_error("tfhe_hip_delete_compressed_packing_key: not a compressed packing key (or already deleted)"); return; }
    key->magic = 0;
    delete key;
}

const uint32_t *tfhe_hip_compressed_packing_key_seed(const TfheHipCompressedPackingKey *key) {
    return compressed_pack_ok("tfhe_hip_compressed_packing_key_seed", key) ? key->seed : nullptr;
}
const Torus32 *tfhe_hip_compressed_packing_key_body(const TfheHipCompressedPackingKey *key, int64_t *count) {
    if (!compressed_pack_ok("tfhe_hip_compressed_packing_key_body", key)) { if (count) *count = 0; return nullptr; }
    if (count) *count = (int64_t)key->body.size();
    return key->body.data();
}
int tfhe_hip_compressed_packing_key_decomposition(const TfheHipCompressedPackingKey *key, int32_t *pk_t, int32_t *pk_basebit) {
    if (!compressed_pack_ok("tfhe_hip_compressed_packing_key_decomposition", key)) return -1;
    if (pk_t) *pk_t = key->t;
    if (pk_basebit) *pk_basebit = key->basebit;
    return 0;
}
int64_t tfhe_hip_compressed_packing_key_bytes(const TfheHipCompressedPackingKey *key) {
    if (!compressed_pack_ok("tfhe_hip_compressed_packing_key_bytes", key)) return -1;
    return (int64_t)(sizeof key->seed + key->body.size() * sizeof(Torus32));
}

TfheHipPackingKey *tfhe_hip_expand_packing_key_host(const TfheHipCompressedPackingKey *key) {
    const char *who = "tfhe_hip_expand_packing_key_host";
    if (!compressed_pack_ok(who, key)) return nullptr;
    TfheHipPackingKey *pk = new_packing_key_object(who, key->p, key->t, key->basebit, false);
    if (pk) expand_packing_rows_host(pk->p, pk->t, key->seed, key->body.data(), pk->rows);
    return pk;
}
TfheHipPackingKey *tfhe_hip_expand_packing_key(const TfheHipCompressedPackingKey *key) {
    const char *who = "tfhe_hip_expand_packing_key";
    if (!compressed_pack_ok(who, key)) return nullptr;
    TfheHipPackingKey *pk = new_packing_key_object(who, key->p, key->t, key->basebit, false);      // no host rows until somebody asks
    if (!pk) return nullptr;
    pk->mask_seed.assign(key->seed, key->seed + 10);
    pk->body = key->body;
    return pk;
}

int tfhe_hip_ring_encrypt_compressed(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, Torus32 *out_words) {
    if (!mu) { set_error("tfhe_hip_ring_encrypt_compressed: null argument"); return -1; }
    return ring_encrypt_compressed_impl("tfhe_hip_ring_encrypt_compressed", secret, mu, nullptr, 0, out_words, nullptr, 0, false);
}
int tfhe_hip_ring_encrypt_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu,
                                            Torus32 *out_words, const uint32_t *mask_seed10, uint64_t noise_seed) {
    if (!mu) { set_error("tfhe_hip_ring_encrypt_compressed_seeded: null argument"); return -1; }
    return ring_encrypt_compressed_impl("tfhe_hip_ring_encrypt_compressed_seeded", secret, mu, nullptr, 0, out_words, mask_seed10,
                                        noise_seed, true);
}
int tfhe_hip_ring_encrypt_bits_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                          Torus32 *out_words) {
    if (!bits) { set_error("tfhe_hip_ring_encrypt_bits_compressed: null argument"); return -1; }
    return ring_encrypt_compressed_impl("tfhe_hip_ring_encrypt_bits_compressed", secret, nullptr, bits, count, out_words, nullptr, 0,
                                        false);
}
int tfhe_hip_ring_encrypt_bits_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits,
                                                 int32_t count, Torus32 *out_words, const uint32_t *mask_seed10,
                                                 uint64_t noise_seed) {
    if (!bits) { set_error("tfhe_hip_ring_encrypt_bits_compressed_seeded: null argument"); return -1; }
    return ring_encrypt_compressed_impl("tfhe_hip_ring_encrypt_bits_compressed_seeded", secret, nullptr, bits, count, out_words,
                                        mask_seed10, noise_seed, true);
}
int tfhe_hip_ring_expand_host(const Torus32 *compressed_words, int32_t N, Torus32 *out_words) {
    if (!compressed_words || !out_words) { set_error("tfhe_hip_ring_expand_host: null argument"); return -1; }
    if (N < 1) { set_error("tfhe_hip_ring_expand_host: N must be at least 1"); return -1; }
    Rng mask = Rng::keyed(reinterpret_cast<const uint32_t *>(compressed_words));
    std::vector<Torus32> body(compressed_words + 10, compressed_words + 10 + N);      // (the two may overlap)
    for (int32_t j = 0; j < N; ++j) out_words[j] = mask.torus();
    std::memcpy(out_words + N, body.data(), (size_t)N * sizeof(Torus32));
    return 0;
}

int tfhe_hip_unpack_samples_seeded(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *compressed_words, int32_t nring,
                                   const int32_t *index, int32_t count, LweSample *result) {
    return guarded_rc([&] { return unpack_impl("tfhe_hip_unpack_samples_seeded", bk, compressed_words, nring, index, count, result, false, true); });
}
int tfhe_hip_unpack_samples_seeded_scattered(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *compressed_words,
                                             int32_t nring, const int32_t *index, int32_t count, LweSample *const *result) {
    return guarded_rc([&] { return unpack_impl("tfhe_hip_unpack_samples_seeded_scattered", bk, compressed_words, nring, index, count, result, false, true); });
}
int tfhe_hip_unpack_samples_seeded_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_compressed_words,
                                          int32_t nring, const int32_t *index, int32_t count, LweSample *result) {
    return guarded_rc([&] { return unpack_impl("tfhe_hip_unpack_samples_seeded_device", bk, static_cast<const Torus32 *>(device_compressed_words), nring, index, count, result, true, true); });
}

int tfhe_hip_kernel_ring_extract_seeded(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *compressed_words, int32_t nring,
                                        const int32_t *index, int32_t count, Torus32 *u_out) {
    return guarded_rc([&] { return ring_extract_impl("tfhe_hip_kernel_ring_extract_seeded", bk, compressed_words, nring, index, count, u_out, true); });
}

int64_t tfhe_hip_test_pack_image(const TfheHipPackingKey *key, const TFheGateBootstrappingCloudKeySet *bk, Torus32 *out,
                                 int64_t capacity) {
    int64_t words = -1;
    guarded([&] {
        const char *who = "tfhe_hip_test_pack_image";
        pack_key_checked(who, key);
        if (!bk || !bk->bk || capacity < 0) api_fail(std::string(who) + ": bad arguments");
        if (!pack_same_set(key->p, bk->bk->p)) api_fail(std::string(who) + ": the cloud key belongs to another parameter set than the packing key");
        auto g = recorder_lock();
        pool_of_key(bk);
        pack_image(key, bk);
        words = (int64_t)Engine::get().read_pack_image(key->img, out, (size_t)capacity);
    });
    return words;
}

int64_t tfhe_hip_test_extract_rows(Torus32 *out, int64_t capacity) {
    if (capacity < 0) { set_error("tfhe_hip_test_extract_rows: bad arguments"); return -1; }
    auto g = recorder_lock();
    return (int64_t)Engine::get().read_extract_rows(out, (size_t)capacity);
}

}  // extern "C"
