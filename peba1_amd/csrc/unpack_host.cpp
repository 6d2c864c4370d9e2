// unpack_host.cpp -- host side of the ring-encrypted inputs: the ring encryption and the C ABI of the unpack
// (include/tfhe_hip.h "ring-encrypted inputs").  No arithmetic of the unpack itself happens here (unpack.hip, then the
// key-switch kernels); encryption runs on the CPU like that of the LWE samples.
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

// ---- what the other host files use (shim_internal.hpp) ----
bool tfhe_hip::ring_message_of_bits(const char *who, const int32_t *bits, int32_t count, int N, std::vector<Torus32> &msg) {
    if (count < 1 || count > N) { set_error(std::string(who) + ": count must be in 1.." + std::to_string(N)); return false; }
    msg.assign((size_t)N, 0);
    for (int32_t j = 0; j < count; ++j) msg[(size_t)j] = bits[j] ? (1 << 29) : -(1 << 29);
    return true;
}

int tfhe_hip::unpack_impl(const char *who, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring, int32_t nring,
                          const int32_t *index, int32_t count, ResultsView result, bool device_src, bool seeded) {
    const std::string w = std::string(who) + ": ";
    if (!ring || !result) api_fail(w + "null ring words or result");
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    const Params &p = bk->bk->p;
    std::vector<int32_t> iota;
    index = ring_index_checked(w, index, count, nring, p.N, true, iota);
    auto g = recorder_lock();
    // every result is ours, of the key's LWE dimension and not bound to the pool of another shape -- before the device is
    // looked at and before anything changes
    check_runs(w, UNPACK_RESULT, result, count, p);
    SlotPool *pool = pool_of_key(bk);
    // a flush in flight owns the key switch's partial sums; what is recorded and has not run stays recorded
    finish_flight_locked();
    import_into_fresh_slots(pool, result, count, [&](const int32_t *slots) {
        Engine::get().run_unpack(bk->bk->dev, ring, nring, device_src, index, count, pool, slots, nullptr, !device_src, seeded);
    });
    return 0;
}

int tfhe_hip::ring_extract_impl(const char *who, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring, int32_t nring,
                                const int32_t *index, int32_t count, Torus32 *u_out, bool seeded) {
    const std::string w = std::string(who) + ": ";
    if (!ring || !u_out) api_fail(w + "null argument");
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    std::vector<int32_t> iota;
    index = ring_index_checked(w, index, count, nring, bk->bk->p.N, false, iota);
    auto g = recorder_lock();
    pool_of_key(bk);
    finish_flight_locked();
    Engine::get().run_unpack(bk->bk->dev, ring, nring, false, index, count, nullptr, nullptr, u_out, true, seeded);
    return 0;
}

namespace {

// The draw order (include/tfhe_hip.h): the kN mask words, then the N noise samples.
void ring_encrypt_into(const TfheHipSecretKey &sk, const Torus32 *mu, Rng &secret, Rng &mask, Torus32 *out) {
    const int N = sk.p.N, k = sk.p.k;
    uint32_t *smp = reinterpret_cast<uint32_t *>(out), *body = smp + (size_t)k * N;
    for (int u = 0; u < k; ++u)
        for (int j = 0; j < N; ++j) smp[(size_t)u * N + j] = (uint32_t)mask.torus();
    for (int j = 0; j < N; ++j) body[j] = (uint32_t)dtot32(secret.gauss(sk.p.bk_stdev)) + (uint32_t)mu[j];
    for (int u = 0; u < k; ++u) pack_add_mul_by_bits(body, smp + (size_t)u * N, sk.tlwe_key.data() + (size_t)u * N, N, 1u);
}

int ring_encrypt_impl(const char *who, const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, const int32_t *bits,
                      int32_t count, Torus32 *out, const uint64_t *seed) {
    if (!secret || !secret->lwe_key || (!mu && !bits) || !out) { set_error(std::string(who) + ": null argument"); return -1; }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    std::vector<Torus32> msg;
    if (bits) {
        if (!ring_message_of_bits(who, bits, count, sk.p.N, msg)) return -1;
        mu = msg.data();
    }
    if (seed) {
        Rng both(*seed);                                  // a stream of its own, for this sample alone
        ring_encrypt_into(sk, mu, both, both, out);
    } else {
        Rng noise = Rng::secure(), mask = Rng::secure();  // two fresh ChaCha20 streams, as for a packing key
        ring_encrypt_into(sk, mu, noise, mask, out);
    }
    return 0;
}

}  // namespace

extern "C" {

int tfhe_hip_ring_encrypt(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, Torus32 *out_words) {
    if (!mu) { set_error("tfhe_hip_ring_encrypt: null argument"); return -1; }
    return ring_encrypt_impl("tfhe_hip_ring_encrypt", secret, mu, nullptr, 0, out_words, nullptr);
}
int tfhe_hip_ring_encrypt_seeded(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, Torus32 *out_words,
                                 uint64_t seed) {
    if (!mu) { set_error("tfhe_hip_ring_encrypt_seeded: null argument"); return -1; }
    return ring_encrypt_impl("tfhe_hip_ring_encrypt_seeded", secret, mu, nullptr, 0, out_words, &seed);
}
int tfhe_hip_ring_encrypt_bits(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                               Torus32 *out_words) {
    if (!bits) { set_error("tfhe_hip_ring_encrypt_bits: null argument"); return -1; }
    return ring_encrypt_impl("tfhe_hip_ring_encrypt_bits", secret, nullptr, bits, count, out_words, nullptr);
}
int tfhe_hip_ring_encrypt_bits_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                      Torus32 *out_words, uint64_t seed) {
    if (!bits) { set_error("tfhe_hip_ring_encrypt_bits_seeded: null argument"); return -1; }
    return ring_encrypt_impl("tfhe_hip_ring_encrypt_bits_seeded", secret, nullptr, bits, count, out_words, &seed);
}

int tfhe_hip_unpack_samples(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                            const int32_t *index, int32_t count, LweSample *result) {
    return guarded_rc([&] { return unpack_impl("tfhe_hip_unpack_samples", bk, ring_words, nring, index, count, result, false); });
}
int tfhe_hip_unpack_samples_scattered(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                                      const int32_t *index, int32_t count, LweSample *const *result) {
    return guarded_rc([&] { return unpack_impl("tfhe_hip_unpack_samples_scattered", bk, ring_words, nring, index, count, result, false); });
}
int tfhe_hip_unpack_samples_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_words, int32_t nring,
                                   const int32_t *index, int32_t count, LweSample *result) {
    return guarded_rc([&] { return unpack_impl("tfhe_hip_unpack_samples_device", bk, static_cast<const Torus32 *>(device_ring_words), nring, index, count, result, true); });
}

int tfhe_hip_kernel_ring_extract(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring,
                                 const int32_t *index, int32_t count, Torus32 *u_out) {
    return guarded_rc([&] { return ring_extract_impl("tfhe_hip_kernel_ring_extract", bk, ring_words, nring, index, count, u_out, false); });
}

}  // extern "C"
