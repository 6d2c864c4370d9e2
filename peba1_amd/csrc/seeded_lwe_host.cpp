// seeded_lwe_host.cpp -- host side of the seed-compressed LWE sample arrays (include/tfhe_hip.h "seed-compressed LWE sample
// arrays"): the array encryptors, the host expansion and the C ABI of the seeded import.  The device side is
// Engine::run_lwe_expand and lwe_expand_kernel (expand.hip).  The encryptors and the host expansion touch neither the
// device nor the recorder.
#include <cstring>
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

namespace {

constexpr RunMessages SEEDED_IMPORT_RESULT{"a result belongs to a parameter set of LWE dimension ", ", the record to one of ",
                                           "count runs past the end of the result array",
                                           "a result lives in the pool of another ciphertext shape"};

bool lwe_record_dimension_ok(const std::string &w, int32_t n) {
    if (n >= 1 && n <= LWE_EXPAND_MAX_N) return true;
    set_error(w + "LWE dimension n must be in [1, " + std::to_string(LWE_EXPAND_MAX_N) + "]");
    return false;
}
bool lwe_record_count_ok(const std::string &w, int32_t record_count) {
    if (record_count >= 1 && record_count <= LWE_RECORD_MAX) return true;
    set_error(w + "a record holds 1.." + std::to_string(LWE_RECORD_MAX) + " samples");
    return false;
}
// count >= 1, and every index inside the record (index null: 0 .. count - 1 must be)
bool lwe_record_index_ok(const std::string &w, const int32_t *index, int32_t count, int32_t record_count) {
    if (count < 1) { set_error(w + "count must be at least 1"); return false; }
    if (!index && count > record_count) { set_error(w + "count runs past the last sample of the record"); return false; }
    for (int32_t j = 0; index && j < count; ++j)
        if (index[j] < 0 || index[j] >= record_count) {
            set_error(w + "index " + std::to_string(index[j]) + " at " + std::to_string(j) + " is outside 0.." + std::to_string(record_count - 1));
            return false;
        }
    return true;
}

// mask_seed10 null: a fresh seed from the OS and fresh noise; else the fixture form.  Mask word i of sample j is draw
// j n + i of the seed's stream; the noise generator yields one gaussian per sample, in order.
int sym_encrypt_compressed_impl(const char *who, const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu,
                                const int32_t *bits, int32_t count, Torus32 *out, const uint32_t *mask_seed10, uint64_t noise_seed,
                                bool fixture) {
    const std::string w = std::string(who) + ": ";
    if (!secret || !secret->lwe_key || (!mu && !bits) || !out || (fixture && !mask_seed10)) { set_error(w + "null argument"); return -1; }
    const TfheHipSecretKey &sk = *secret->lwe_key;
    if (!lwe_record_dimension_ok(w, sk.p.n) || !lwe_record_count_ok(w, count)) return -1;
    uint32_t seed[LWE_SEED_WORDS];
    if (fixture) std::memcpy(seed, mask_seed10, sizeof seed);
    else os_seed(seed);
    Rng mask = Rng::keyed(seed);
    Rng noise = fixture ? Rng(noise_seed) : Rng::secure();
    std::vector<uint32_t> body((size_t)count);             // (mu may alias out)
    for (int32_t j = 0; j < count; ++j) {
        const uint32_t m = bits ? (bits[j] ? 1u << 29 : 0u - (1u << 29)) : (uint32_t)mu[j];
        uint32_t b = m + (uint32_t)dtot32(noise.gauss(sk.p.ks_stdev));
        for (int32_t i = 0; i < sk.p.n; ++i) b += (uint32_t)mask.torus() * (uint32_t)sk.lwe_key[(size_t)i];
        body[(size_t)j] = b;
    }
    std::memcpy(out, seed, sizeof seed);
    std::memcpy(out + LWE_SEED_WORDS, body.data(), (size_t)count * 4);
    return 0;
}

int import_seeded_impl(const char *who, const TFheGateBootstrappingParameterSet *params, const Torus32 *record, int32_t record_count,
                       const int32_t *index, int32_t count, ResultsView result, bool device_src) {
    const std::string w = std::string(who) + ": ";
    if (!record || !result) api_fail(w + "null record words or result");
    if (!params || !params->in_out_params) api_fail(w + "null parameter set");
    const Params &p = params_of(params);
    if (!lwe_record_dimension_ok(w, p.n) || !lwe_record_count_ok(w, record_count) || !lwe_record_index_ok(w, index, count, record_count))
        api_fail(last_error_ref());
    std::vector<int32_t> iota;
    index = index_or_iota(index, count, iota);
    auto g = recorder_lock();
    // every result is ours, of the set's LWE dimension and not bound to the pool of another shape -- before the device is
    // looked at and before anything changes
    check_runs(w, SEEDED_IMPORT_RESULT, result, count, p);
    SlotPool *pool = Engine::get().pool_for(p);
    // what is recorded and has not run stays recorded: it cannot name the new slots
    finish_flight_locked();
    import_into_fresh_slots(pool, result, count, [&](const int32_t *slots) {
        Engine::get().run_lwe_expand(p.n, p.ct_stride(), record, device_src, index, count, pool, slots, nullptr, !device_src);
    });
    return 0;
}

}  // namespace

extern "C" {

int tfhe_hip_sym_encrypt_bits_compressed(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                         Torus32 *out_words) {
    if (!bits) { set_error("tfhe_hip_sym_encrypt_bits_compressed: null argument"); return -1; }
    return sym_encrypt_compressed_impl("tfhe_hip_sym_encrypt_bits_compressed", secret, nullptr, bits, count, out_words, nullptr, 0, false);
}
int tfhe_hip_sym_encrypt_bits_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const int32_t *bits, int32_t count,
                                                Torus32 *out_words, const uint32_t *mask_seed10, uint64_t noise_seed) {
    if (!bits) { set_error("tfhe_hip_sym_encrypt_bits_compressed_seeded: null argument"); return -1; }
    return sym_encrypt_compressed_impl("tfhe_hip_sym_encrypt_bits_compressed_seeded", secret, nullptr, bits, count, out_words,
                                       mask_seed10, noise_seed, true);
}
int tfhe_hip_sym_encrypt_torus_compressed(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, int32_t count,
                                          Torus32 *out_words) {
    if (!mu) { set_error("tfhe_hip_sym_encrypt_torus_compressed: null argument"); return -1; }
    return sym_encrypt_compressed_impl("tfhe_hip_sym_encrypt_torus_compressed", secret, mu, nullptr, count, out_words, nullptr, 0, false);
}
int tfhe_hip_sym_encrypt_torus_compressed_seeded(const TFheGateBootstrappingSecretKeySet *secret, const Torus32 *mu, int32_t count,
                                                 Torus32 *out_words, const uint32_t *mask_seed10, uint64_t noise_seed) {
    if (!mu) { set_error("tfhe_hip_sym_encrypt_torus_compressed_seeded: null argument"); return -1; }
    return sym_encrypt_compressed_impl("tfhe_hip_sym_encrypt_torus_compressed_seeded", secret, mu, nullptr, count, out_words,
                                       mask_seed10, noise_seed, true);
}

// The stream is addressed by block: sample s starts at word s n, in block s n / 8.  One sample after the other, each from
// its first block on, so that a caller who asks for the last sample of a large record pays for that sample alone.
int tfhe_hip_lwe_expand_host(const Torus32 *compressed_words, int32_t n, int32_t record_count, const int32_t *index, int32_t count,
                             Torus32 *out_words) {
    const std::string w = "tfhe_hip_lwe_expand_host: ";
    if (!compressed_words || !out_words) { set_error(w + "null argument"); return -1; }
    if (!lwe_record_dimension_ok(w, n) || !lwe_record_count_ok(w, record_count) || !lwe_record_index_ok(w, index, count, record_count))
        return -1;
    const uint32_t *seed = reinterpret_cast<const uint32_t *>(compressed_words);
    for (int32_t j = 0; j < count; ++j) {
        const int64_t s = index ? index[j] : j;
        Torus32 *row = out_words + (size_t)j * ((size_t)n + 1);
        uint32_t block[16];
        int64_t have = -1;                                 // the block `block` holds
        for (int32_t i = 0; i < n; ++i) {
            const int64_t m = s * n + i;
            if (m / 8 != have) { have = m / 8; Rng::chacha_block(seed, (uint64_t)have, seed + 8, block); }
            row[i] = (Torus32)block[2 * (m % 8) + 1];
        }
        row[n] = compressed_words[LWE_SEED_WORDS + s];
    }
    return 0;
}

int tfhe_hip_import_samples_seeded(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words,
                                   int32_t record_count, const int32_t *index, int32_t count, LweSample *result) {
    return guarded_rc([&] { return import_seeded_impl("tfhe_hip_import_samples_seeded", params, compressed_words, record_count, index, count, result, false); });
}
int tfhe_hip_import_samples_seeded_scattered(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words,
                                             int32_t record_count, const int32_t *index, int32_t count, LweSample *const *result) {
    return guarded_rc([&] { return import_seeded_impl("tfhe_hip_import_samples_seeded_scattered", params, compressed_words, record_count, index, count, result, false); });
}
int tfhe_hip_import_samples_seeded_device(const TFheGateBootstrappingParameterSet *params, const void *device_compressed_words,
                                          int32_t record_count, const int32_t *index, int32_t count, LweSample *result) {
    return guarded_rc([&] { return import_seeded_impl("tfhe_hip_import_samples_seeded_device", params, static_cast<const Torus32 *>(device_compressed_words), record_count, index, count, result, true); });
}

int tfhe_hip_kernel_lwe_expand(const TFheGateBootstrappingParameterSet *params, const Torus32 *compressed_words, int32_t record_count,
                               const int32_t *index, int32_t count, Torus32 *out_words) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_lwe_expand: ";
        if (!compressed_words || !out_words) api_fail(w + "null argument");
        if (!params || !params->in_out_params) api_fail(w + "null parameter set");
        const Params &p = params_of(params);
        if (!lwe_record_dimension_ok(w, p.n) || !lwe_record_count_ok(w, record_count) || !lwe_record_index_ok(w, index, count, record_count))
            api_fail(last_error_ref());
        std::vector<int32_t> iota;
        index = index_or_iota(index, count, iota);
        auto g = recorder_lock();
        finish_flight_locked();
        Engine::get().run_lwe_expand(p.n, p.ct_stride(), compressed_words, false, index, count, nullptr, nullptr, out_words, true);
        return 0;
    });
}

int64_t tfhe_hip_test_expand_slots(Torus32 *out, int64_t capacity) {
    if (capacity < 0) { set_error("tfhe_hip_test_expand_slots: bad arguments"); return -1; }
    auto g = recorder_lock();
    return (int64_t)Engine::get().read_expand_slots(out, (size_t)capacity);
}

void tfhe_hip_get_seeded_lwe_stats(TfheHipSeededLweStats *out) {
    auto g = recorder_lock();
    if (out) *out = Engine::get().seeded_lwe_stats;
}

}  // extern "C"
