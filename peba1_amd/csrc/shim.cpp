// shim.cpp -- the C ABI of libtfhe-hip: the tfhe boots* surface that
// /root/reference/src/Math.cpp and src/main.cpp bind plus the
// tfhe_hip_* extensions.  Host logic only: the array headers, keys, I/O glue, tunings and statistics; the
// boots* gate entries hand over to the recorder (recorder.hpp).  No gate arithmetic happens here.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "br_forms.hpp"
#include "engine.hpp"
#include "op_graph.hpp"
#include "recorder.hpp"
#include "scheduler.hpp"
#include "../../include/tfhe/tfhe.h"

using namespace tfhe_hip;

namespace tfhe_hip {
const std::string &last_error_ref();
bool io_forget_owned_cloud(const void *ks);     // io.cpp: keysets created by the file loaders
bool io_forget_owned_secret(const void *ks);
TFheGateBootstrappingCloudKeySet *io_adopt_cloud(TfheHipCloudKey *ck);   // io.cpp: a cloud keyset of its own around ck
}

namespace {

constexpr uint32_t ARRAY_MAGIC = 0x7F4E11A5u;

// Hidden header in front of every LweSample array handed to the caller.
struct alignas(16) ArrayHeader {
    uint32_t magic;
    int32_t count;
    int32_t n;
    int32_t unused;
    SlotPool *pool;     // set when the first element moves to the device
};

// Every sample's host mirror is preceded by a back-pointer to its array's header and a marker, so
// the pool a sample lives in can be found from any element pointer (&array[i]).  The marker is
// checked BEFORE the back-pointer is followed.  Why it matters: the reference's Function_g writes
// bitsize+1 results into a bitsize-sample array (Math.cpp:399-401).  That "sample" one
// past the end overlays the first mirror prefix of the block, so its `a` field reads as the
// back-pointer (the block's own start): the words in front of THAT are the allocator's chunk header
// -- readable, and not the marker -- and the call is refused instead of following garbage.
constexpr int MIRROR_PREFIX_WORDS = 4;   // one pointer + marker (8 bytes)
constexpr uint64_t MIRROR_MARKER = 0x7F4E5A3D1E5AA11Cull;

ArrayHeader *header_of(const LweSample *sample) {
    uint64_t marker;
    ArrayHeader *h;
    if (!sample || !sample->a) api_fail("LweSample was not allocated by new_gate_bootstrapping_ciphertext_array");
    std::memcpy(&marker, sample->a - 2, sizeof marker);
    if (marker != MIRROR_MARKER) api_fail("LweSample was not allocated by new_gate_bootstrapping_ciphertext_array");
    std::memcpy(&h, sample->a - MIRROR_PREFIX_WORDS, sizeof h);
    if (!h || h->magic != ARRAY_MAGIC) api_fail("LweSample was not allocated by new_gate_bootstrapping_ciphertext_array");
    return h;
}

// Argument checks the pack and unpack entries share (pack_host.cpp, unpack_host.cpp); w: "entry name: ".
// Each of the `runs` runs of `count` consecutive samples from first_of(j) lies inside one array of ours, of LWE dimension
// p.n and not bound to the pool of another ciphertext shape: the arrays first, then the pools, in the caller's words.
// Never initialises the device.
struct RunMessages { const char *dimension, *key_has, *past_end, *other_pool; };
constexpr RunMessages PACK_SAMPLES{"the samples belong to a parameter set of LWE dimension ", ", the packing key to one of ",
                                   "count runs past the end of the samples' array",
                                   "the samples live in the pool of another ciphertext shape"};
constexpr RunMessages UNPACK_RESULT{"a result belongs to a parameter set of LWE dimension ", ", the cloud key to one of ",
                                    "count runs past the end of the result array",
                                    "a result lives in the pool of another ciphertext shape"};
template <typename At>
void check_runs(const std::string &w, const RunMessages &say, At first_of, int32_t runs, int32_t count, const Params &p) {
    for (int32_t j = 0; j < runs; ++j) {
        const LweSample *first = first_of(j);
        if (!first) api_fail(w + "null result sample at " + std::to_string(j));
        const ArrayHeader *h = header_of(first);          // (refuses a foreign sample)
        if (h->n != p.n) api_fail(w + say.dimension + std::to_string(h->n) + say.key_has + std::to_string(p.n));
        if (first - reinterpret_cast<const LweSample *>(reinterpret_cast<const char *>(h) + sizeof(ArrayHeader)) + count > h->count)
            api_fail(w + say.past_end);
    }
    const SlotPool *pool = Engine::get().find_pool(p);
    for (int32_t j = 0; j < runs; ++j)
        if (const SlotPool *bound = header_of(first_of(j))->pool; bound && bound != pool) api_fail(w + say.other_pool);
}
// The coefficient list of an unpack of nring ring samples of N: every index inside them, or -- index null -- 0 .. count - 1,
// which `iota` then holds.  at: the refusal of an index names its position and the range
const int32_t *ring_index_checked(const std::string &w, const int32_t *index, int32_t count, int32_t nring, int32_t N, bool at,
                                  std::vector<int32_t> &iota) {
    if (count < 1 || nring < 1) api_fail(w + "count and nring must be at least 1");
    const int64_t ncoef = (int64_t)nring * N;
    if (ncoef > INT32_MAX) api_fail(w + "nring * N must stay below 2^31");
    if (!index && count > ncoef) api_fail(w + "count runs past the last coefficient of the ring samples");
    for (int32_t j = 0; index && j < count; ++j)
        if (index[j] < 0 || index[j] >= ncoef)
            api_fail(at ? w + "index " + std::to_string(index[j]) + " at " + std::to_string(j) + " is outside 0.." + std::to_string(ncoef - 1)
                        : w + "index " + std::to_string(index[j]) + " is out of range");
    if (index) return index;
    iota.resize((size_t)count);
    std::iota(iota.begin(), iota.end(), 0);
    return iota.data();
}

// Every extern "C" entry runs its body through one of these: an ApiError becomes
// tfhe_hip_last_error() and the call has no effect (void entries) or returns -1.
template <typename F>
void guarded(F &&body) {
    try { body(); } catch (const ApiError &e) { set_error(e.msg); }
}
template <typename F>
int guarded_rc(F &&body) {
    try { return body(); } catch (const ApiError &e) { set_error(e.msg); return -1; }
}

// Every *_batch entry: `body` records its ops deferred whatever the caller's mode; a caller in immediate mode has them run
// before the call returns -- those recorded before a refused one included.
template <typename F>
int record_batch(F &&body) {
    auto g = recorder_lock();
    const bool was = set_deferred_locked(true);
    const int rc = guarded_rc([&] { body(); return 0; });
    set_deferred_locked(was);
    if (!was) flush_locked();
    return rc;
}

void record_gate2(int code, LweSample *result, const LweSample *ca, const LweSample *cb,
                  const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        record_gate2_locked(code, result, ca, cb, bk);
    });
}

// bootsSymEncrypt and the default keygen draw from two ChaCha20 streams keyed by the OS (host_keys.hpp: one for the noise /
// the secrets, one for the public masks); after tfhe_hip_set_encrypt_seed both roles fall to ONE seeded xoshiro generator
// (secret; the specified draw order of the fixtures).  Used under the recorder lock.
struct EncryptRng { Rng secret = Rng::secure(), mask = Rng::secure(); bool seeded = false; };
EncryptRng &enc_rng() { static EncryptRng e; return e; }

}  // namespace

// one array never spans two pools
void tfhe_hip::bind_pool(const LweSample *sample, SlotPool *pool) {
    ArrayHeader *h = header_of(sample);
    if (!h->pool) h->pool = pool;
    else if (h->pool != pool) api_fail("ciphertext used with a key of different LWE dimension than the one it was first used with");
}
SlotPool *tfhe_hip::pool_of_sample(const LweSample *sample) { return header_of(sample)->pool; }

// ===========================================================================
// upstream-compatible C ABI
// ===========================================================================
extern "C" {

int32_t modSwitchFromTorus32(Torus32 phase, int32_t Msize) {
    const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
    const uint64_t phase64 = ((uint64_t)(uint32_t)phase << 32) + interv / 2;
    return (int32_t)(phase64 / interv);
}
Torus32 modSwitchToTorus32(int32_t mu, int32_t Msize) {
    const uint64_t interv = ((UINT64_C(1) << 63) / (uint64_t)Msize) * 2;
    return (Torus32)(((uint64_t)(int64_t)mu * interv) >> 32);
}

TFheGateBootstrappingParameterSet *new_default_gate_bootstrapping_parameters(int32_t minimum_lambda) {
    Params p;
    if (!default_params(minimum_lambda, p)) {
        std::fprintf(stderr, "Sorry, for now, the parameters are only implemented for 80bit and 128bit of security!\n");
        set_error("unsupported minimum_lambda");
        return nullptr;
    }
    return &make_param_bundle(p)->set;
}

void delete_gate_bootstrapping_parameters(TFheGateBootstrappingParameterSet *params) {
    delete reinterpret_cast<ParamBundle *>(params);
}

// seed == nullptr: secrets and masks from two ChaCha20 streams keyed by the OS; else the seeded generator (fixtures)
static TFheGateBootstrappingSecretKeySet *make_keyset(const TFheGateBootstrappingParameterSet *params, const uint64_t *seed,
                                                      bool device) {
    if (!params) { set_error("null params"); return nullptr; }
    const Params &p = params_of(params);
    auto *sk = new TfheHipSecretKey();
    auto *ck = new TfheHipCloudKey();
    if (seed) {
        Rng both(*seed);
        generate_keys(p, both, both, *sk, *ck);
    } else {
        Rng secret = Rng::secure(), mask = Rng::secure();
        generate_keys(p, secret, mask, *sk, *ck);
    }
    if (device) {
        try {
            ck->dev = Engine::get().upload_key(*ck);
        } catch (const ApiError &e) {       // a parameter set the kernels cannot run exactly: no keyset, and why
            set_error(e.msg);
            delete sk;
            delete ck;
            return nullptr;
        }
    }
    auto *ks = new TFheGateBootstrappingSecretKeySet();
    ks->params = params;
    ks->lwe_key = sk;
    ks->tgsw_key = sk;
    ks->cloud.params = params;
    ks->cloud.bk = ck;
    ks->cloud.bkFFT = ck;
    return ks;
}

TFheGateBootstrappingSecretKeySet *new_random_gate_bootstrapping_secret_keyset(const TFheGateBootstrappingParameterSet *params) {
    // upstream draws from its global generator; here every keyset comes from ChaCha20 streams keyed with 256 bits
    // of OS entropy each (reproducible keys: tfhe_hip_new_secret_keyset_seeded)
    return make_keyset(params, nullptr, true);
}

void delete_gate_bootstrapping_secret_keyset(TFheGateBootstrappingSecretKeySet *keyset) {
    if (!keyset) return;
    auto g = recorder_lock();
    forget_key_locked(&keyset->cloud);
    if (keyset->cloud.bk) {
        Engine::get().free_key(keyset->cloud.bk->dev);
        delete keyset->cloud.bk;
    }
    delete keyset->lwe_key;
    if (io_forget_owned_secret(keyset)) delete_gate_bootstrapping_parameters(const_cast<TFheGateBootstrappingParameterSet *>(keyset->params));
    delete keyset;
}

void delete_gate_bootstrapping_cloud_keyset(TFheGateBootstrappingCloudKeySet *keyset) {
    // A cloud keyset embedded in a secret keyset (&key->cloud, main.cpp:23) goes with its owner;
    // only one created by new_tfheGateBootstrappingCloudKeySet_fromFile is released here.
    if (!keyset || !io_forget_owned_cloud(keyset)) return;
    auto g = recorder_lock();
    forget_key_locked(keyset);
    if (keyset->bk) {
        Engine::get().free_key(keyset->bk->dev);
        delete keyset->bk;
    }
    delete_gate_bootstrapping_parameters(const_cast<TFheGateBootstrappingParameterSet *>(keyset->params));
    delete keyset;
}

LweSample *new_gate_bootstrapping_ciphertext_array(int32_t nbelems, const TFheGateBootstrappingParameterSet *params) {
    if (nbelems < 0 || !params) { set_error("bad arguments to new_gate_bootstrapping_ciphertext_array"); return nullptr; }
    const int32_t n = params->in_out_params->n;
    const size_t mirror = (size_t)(n + MIRROR_PREFIX_WORDS + 1) & ~(size_t)1;   // words per sample, pointer-aligned
    const size_t bytes = sizeof(ArrayHeader) + (size_t)nbelems * sizeof(LweSample) + (size_t)nbelems * mirror * sizeof(Torus32);
    char *mem = static_cast<char *>(std::calloc(1, bytes));
    if (!mem) fatal("out of host memory");
    auto *h = reinterpret_cast<ArrayHeader *>(mem);
    h->magic = ARRAY_MAGIC; h->count = nbelems; h->n = n; h->pool = nullptr;
    auto *samples = reinterpret_cast<LweSample *>(mem + sizeof(ArrayHeader));
    auto *words = reinterpret_cast<Torus32 *>(mem + sizeof(ArrayHeader) + (size_t)nbelems * sizeof(LweSample));
    for (int32_t i = 0; i < nbelems; ++i) {
        samples[i].a = words + (size_t)i * mirror + MIRROR_PREFIX_WORDS;
        std::memcpy(samples[i].a - MIRROR_PREFIX_WORDS, &h, sizeof h);
        std::memcpy(samples[i].a - 2, &MIRROR_MARKER, sizeof MIRROR_MARKER);
        samples[i].b = -(1 << 29);      // fresh = trivial encryption of 0, like bootsCONSTANT(.., 0)
        samples[i].slot = SLOT_ZERO;
        samples[i].current_variance = 0.0;
    }
    return samples;
}

void delete_gate_bootstrapping_ciphertext_array(int32_t nbelems, LweSample *samples) {
    if (!samples) return;
    auto *h = reinterpret_cast<ArrayHeader *>(reinterpret_cast<char *>(samples) - sizeof(ArrayHeader));
    if (h->magic != ARRAY_MAGIC) {      // not ours (or already freed): report, leak rather than abort
        set_error("delete_gate_bootstrapping_ciphertext_array: not an array base pointer");
        return;
    }
    if (h->count != nbelems) set_error("delete_gate_bootstrapping_ciphertext_array: count differs from allocation");
    auto g = recorder_lock();
    for (int32_t i = 0; i < h->count; ++i)
        if (samples[i].slot >= 0) h->pool->release(samples[i].slot);
    h->magic = 0;
    std::free(h);
}

LweSample *new_gate_bootstrapping_ciphertext(const TFheGateBootstrappingParameterSet *params) {
    return new_gate_bootstrapping_ciphertext_array(1, params);
}
void delete_gate_bootstrapping_ciphertext(LweSample *sample) { delete_gate_bootstrapping_ciphertext_array(1, sample); }

void bootsSymEncrypt(LweSample *result, int32_t message, const TFheGateBootstrappingSecretKeySet *key) {
    guarded([&] {
        auto g = recorder_lock();
        EncryptRng &e = enc_rng();
        if (result->slot >= 0) header_of(result)->pool->release(result->slot);
        result->slot = SLOT_HOST;
        encrypt_bit(*key->lwe_key, e.secret, e.seeded ? e.secret : e.mask, message, result->a, &result->b);
    });
}

int32_t bootsSymDecrypt(const LweSample *sample, const TFheGateBootstrappingSecretKeySet *key) {
    int32_t bit = 0;
    guarded([&] {
        auto g = recorder_lock();
        sync_sample_locked(sample);
        bit = phase_of(*key->lwe_key, sample->a, sample->b) > 0 ? 1 : 0;
    });
    return bit;
}

// bootsSymEncrypt's path with any message: the same deviation, the same streams, the same draw order
void tfhe_hip_sym_encrypt_torus(LweSample *result, Torus32 mu, const TFheGateBootstrappingSecretKeySet *key) {
    guarded([&] {
        if (!key || !key->lwe_key) api_fail("tfhe_hip_sym_encrypt_torus: null key");
        auto g = recorder_lock();
        EncryptRng &e = enc_rng();
        ArrayHeader *h = header_of(result);                  // (refuses a null or foreign sample)
        if (h->n != key->lwe_key->p.n) api_fail("tfhe_hip_sym_encrypt_torus: the sample and the key differ in LWE dimension");
        if (result->slot >= 0) h->pool->release(result->slot);
        result->slot = SLOT_HOST;
        encrypt_torus(*key->lwe_key, e.secret, e.seeded ? e.secret : e.mask, mu, result->a, &result->b);
    });
}

Torus32 tfhe_hip_sym_phase(const LweSample *sample, const TFheGateBootstrappingSecretKeySet *key) {
    Torus32 phase = 0;
    guarded([&] {
        if (!key || !key->lwe_key) api_fail("tfhe_hip_sym_phase: null key");
        auto g = recorder_lock();
        if (header_of(sample)->n != key->lwe_key->p.n) api_fail("tfhe_hip_sym_phase: the sample and the key differ in LWE dimension");
        sync_sample_locked(sample);
        phase = phase_of(*key->lwe_key, sample->a, sample->b);
    });
    return phase;
}

void bootsCONSTANT(LweSample *result, int32_t value, const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        record_constant_locked(result, value, bk);
    });
}

void bootsCOPY(LweSample *result, const LweSample *ca, const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        record_copy_locked(result, ca, bk);
    });
}

void bootsNOT(LweSample *result, const LweSample *ca, const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        record_not_locked(result, ca, bk);
    });
}

void bootsNAND(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_NAND, r_, a, b, bk); }
void bootsOR(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_OR, r_, a, b, bk); }
void bootsAND(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_AND, r_, a, b, bk); }
void bootsNOR(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_NOR, r_, a, b, bk); }
void bootsXOR(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_XOR, r_, a, b, bk); }
void bootsXNOR(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_XNOR, r_, a, b, bk); }
void bootsANDNY(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_ANDNY, r_, a, b, bk); }
void bootsANDYN(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_ANDYN, r_, a, b, bk); }
void bootsORNY(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_ORNY, r_, a, b, bk); }
void bootsORYN(LweSample *r_, const LweSample *a, const LweSample *b, const TFheGateBootstrappingCloudKeySet *bk) { record_gate2(TFHE_HIP_ORYN, r_, a, b, bk); }

void bootsMUX(LweSample *result, const LweSample *a, const LweSample *b, const LweSample *c,
              const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        record_mux_locked(result, a, b, c, bk);
    });
}

// ===========================================================================
// tfhe_hip_* extensions
// ===========================================================================
const char *tfhe_hip_last_error(void) { return last_error_ref().c_str(); }
void tfhe_hip_clear_error(void) { set_error(""); }

int tfhe_hip_set_device(int device) { Engine::get().set_device(device); return 0; }
int tfhe_hip_get_device(void) { return Engine::get().device(); }

TFheGateBootstrappingParameterSet *tfhe_hip_new_parameters(int32_t n, int32_t N, int32_t k, int32_t l, int32_t Bgbit,
                                                           int32_t ks_t, int32_t ks_basebit, double ks_stdev,
                                                           double bk_stdev, double max_stdev) {
    if (n <= 0 || N <= 0 || (N & (N - 1)) || k < 1 || l < 1 || Bgbit < 1 || l * Bgbit > 32 || ks_t < 1 ||
        ks_basebit < 1 || ks_t * ks_basebit > 31) {
        set_error("tfhe_hip_new_parameters: invalid parameter tuple");
        return nullptr;
    }
    Params p{n, N, k, l, Bgbit, ks_t, ks_basebit, ks_stdev, bk_stdev, max_stdev};
    return &make_param_bundle(p)->set;
}
TFheGateBootstrappingParameterSet *tfhe_hip_new_p2048_parameters(void) { return &make_param_bundle(p2048_params())->set; }

TFheGateBootstrappingSecretKeySet *tfhe_hip_new_secret_keyset_seeded(const TFheGateBootstrappingParameterSet *params, uint64_t seed) {
    return make_keyset(params, &seed, true);
}
TFheGateBootstrappingSecretKeySet *tfhe_hip_new_secret_keyset_seeded_host(const TFheGateBootstrappingParameterSet *params, uint64_t seed) {
    return make_keyset(params, &seed, false);
}
void tfhe_hip_test_chacha20_block(const uint32_t *key8, uint64_t counter, const uint32_t *nonce2, uint32_t *out16) {
    Rng::chacha_block(key8, counter, nonce2, out16);
}
int tfhe_hip_randomness_is_seeded(void) {
    auto g = recorder_lock();
    return enc_rng().seeded ? 1 : 0;
}
void tfhe_hip_set_encrypt_seed(uint64_t seed) {
    auto g = recorder_lock();
    enc_rng().secret.reseed(seed);
    enc_rng().seeded = true;
}

const int32_t *tfhe_hip_key_lwe(const TFheGateBootstrappingSecretKeySet *key, int64_t *count) {
    if (count) *count = (int64_t)key->lwe_key->lwe_key.size();
    return key->lwe_key->lwe_key.data();
}
const int32_t *tfhe_hip_key_tlwe(const TFheGateBootstrappingSecretKeySet *key, int64_t *count) {
    if (count) *count = (int64_t)key->lwe_key->tlwe_key.size();
    return key->lwe_key->tlwe_key.data();
}
// (a device-expanded keyset gets its host words here, under the library's lock, the first time they are asked for)
const Torus32 *tfhe_hip_key_bk(const TFheGateBootstrappingCloudKeySet *cloud, int64_t *count) {
    { auto g = recorder_lock(); materialise_host_words(*const_cast<TfheHipCloudKey *>(cloud->bk)); }
    if (count) *count = (int64_t)cloud->bk->bk.size();
    return cloud->bk->bk.data();
}
const Torus32 *tfhe_hip_key_ksk(const TFheGateBootstrappingCloudKeySet *cloud, int64_t *count) {
    { auto g = recorder_lock(); materialise_host_words(*const_cast<TfheHipCloudKey *>(cloud->bk)); }
    if (count) *count = (int64_t)cloud->bk->ksk.size();
    return cloud->bk->ksk.data();
}

int32_t tfhe_hip_sample_words(const TFheGateBootstrappingParameterSet *params) { return params->in_out_params->n + 1; }

// The pool a group of samples lives in (or will live in): the one their array is already
// bound to, else the pool of this parameter set's ciphertext shape if the engine has one, else --
// only when `create` (a device-side transfer needs one) -- a new pool.  nullptr = no device
// state for this shape yet: the host mirrors are authoritative.
static SlotPool *resolve_pool(const LweSample *samples, const TFheGateBootstrappingParameterSet *params, bool create) {
    if (!params || !params->in_out_params) api_fail("null parameter set");
    const Params &p = params_of(params);
    SlotPool *bound = header_of(samples)->pool;
    if (bound) {
        if (bound->ct_words() != p.ct_words())
            api_fail("samples belong to a parameter set of LWE dimension " + std::to_string(bound->ct_words() - 1) +
                     ", not " + std::to_string(p.n));
        return bound;
    }
    if (SlotPool *pl = Engine::get().find_pool(p)) return pl;
    return create ? Engine::get().pool_for(p) : nullptr;
}

static int export_impl(const LweSample *samples, int32_t count, const TFheGateBootstrappingParameterSet *params,
                       Torus32 *out, bool device_dst, bool wait = true) {
    auto g = recorder_lock();
    if (count <= 0) return 0;
    const int32_t n = params_of(params).n;
    SlotPool *pool = resolve_pool(samples, params, device_dst);
    bool any_dev = false;
    for (int32_t i = 0; i < count; ++i) any_dev |= samples[i].slot >= 0;
    if (!device_dst && (!any_dev || !pool)) {
        for (int32_t i = 0; i < count; ++i) {
            if (samples[i].slot == SLOT_ZERO) {          // fresh: trivial encryption of 0
                std::memset(out + (size_t)i * (n + 1), 0, (size_t)n * 4);
                out[(size_t)i * (n + 1) + n] = -(1 << 29);
                continue;
            }
            std::memcpy(out + (size_t)i * (n + 1), samples[i].a, (size_t)n * 4);
            out[(size_t)i * (n + 1) + n] = samples[i].b;
        }
        return 0;
    }
    // the stream-ordered form (wait == false) only ENQUEUES the pending gates' launches: the gather below, and whatever
    // the caller puts on the stream after it (a collective), follow them in stream order with no host wait (ADVICE r4:
    // a synchronous flush here made every rank of a sharded match sit out its whole local phase on the host)
    flush_pending_locked(wait);
    std::vector<int32_t> slots(count);
    for (int32_t i = 0; i < count; ++i) slots[i] = ensure_slot(&samples[i], pool);
    Engine::get().read_slots_packed(pool, slots.data(), count, out, device_dst, wait);
    return 0;
}

static int import_impl(LweSample *samples, int32_t count, const TFheGateBootstrappingParameterSet *params,
                       const Torus32 *in, bool device_src, bool wait = true) {
    auto g = recorder_lock();
    if (count <= 0) return 0;
    const int32_t n = params_of(params).n;
    SlotPool *pool = resolve_pool(samples, params, device_src);
    if (!pool) {                                         // no device state for this shape: host mirrors only
        for (int32_t i = 0; i < count; ++i) {
            std::memcpy(samples[i].a, in + (size_t)i * (n + 1), (size_t)n * 4);
            samples[i].b = in[(size_t)i * (n + 1) + n];
            samples[i].slot = SLOT_HOST;
        }
        return 0;
    }
    // refuse before anything changes (Engine::write_slots_packed would refuse the count with the slots already taken)
    if (count > MAX_PACKED_SAMPLES) api_fail("too many samples in one packed transfer");
    for (int32_t i = 0; i < count; ++i) bind_pool(&samples[i], pool);
    std::vector<int32_t> slots(count);
    for (int32_t i = 0; i < count; ++i) {
        repoint(&samples[i], pool, alloc_slot(pool));
        slots[i] = samples[i].slot;
        if (!device_src) {
            std::memcpy(samples[i].a, in + (size_t)i * (n + 1), (size_t)n * 4);
            samples[i].b = in[(size_t)i * (n + 1) + n];
        }
    }
    Engine::get().write_slots_packed(pool, slots.data(), count, in, device_src, wait);
    return 0;
}

int tfhe_hip_export_samples(const LweSample *samples, int32_t count, const TFheGateBootstrappingParameterSet *params,
                            Torus32 *out_words) {
    return guarded_rc([&] { return export_impl(samples, count, params, out_words, false); });
}
int tfhe_hip_import_samples(LweSample *samples, int32_t count, const TFheGateBootstrappingParameterSet *params,
                            const Torus32 *in_words) {
    return guarded_rc([&] { return import_impl(samples, count, params, in_words, false); });
}
int tfhe_hip_export_samples_device(const LweSample *samples, int32_t count,
                                   const TFheGateBootstrappingParameterSet *params, void *device_words) {
    return guarded_rc([&] { return export_impl(samples, count, params, static_cast<Torus32 *>(device_words), true); });
}
int tfhe_hip_import_samples_device(LweSample *samples, int32_t count, const TFheGateBootstrappingParameterSet *params,
                                   const void *device_words) {
    return guarded_rc([&] { return import_impl(samples, count, params, static_cast<const Torus32 *>(device_words), true); });
}

int tfhe_hip_export_samples_device_async(const LweSample *samples, int32_t count,
                                         const TFheGateBootstrappingParameterSet *params, void *device_words) {
    return guarded_rc([&] { return export_impl(samples, count, params, static_cast<Torus32 *>(device_words), true, false); });
}
int tfhe_hip_import_samples_device_async(LweSample *samples, int32_t count, const TFheGateBootstrappingParameterSet *params,
                                         const void *device_words) {
    return guarded_rc([&] { return import_impl(samples, count, params, static_cast<const Torus32 *>(device_words), true, false); });
}
void *tfhe_hip_stream(void) {
    Engine::get().ensure_init();
    return static_cast<void *>(Engine::get().stream());
}

int tfhe_hip_sync_samples(const LweSample *samples, int32_t count) {
    return guarded_rc([&] {
        auto g = recorder_lock();
        flush_pending_locked();
        for (int32_t i = 0; i < count; ++i) sync_sample_locked(&samples[i]);
        return 0;
    });
}

void tfhe_hip_set_deferred(int on) {
    auto g = recorder_lock();
    if (!on) guarded([&] { flush_pending_locked(); });
    set_deferred_locked(on != 0);
}
int tfhe_hip_get_deferred(void) { return deferred_mode() ? 1 : 0; }

int tfhe_hip_flush(void) {
    auto g = recorder_lock();
    return guarded_rc([&] { return flush_locked(); });
}
int tfhe_hip_flush_async(void) {
    auto g = recorder_lock();
    return guarded_rc([&] { return flush_locked(false); });
}
int tfhe_hip_wait(void) {
    auto g = recorder_lock();
    // the flush in flight, and the stream-ordered transfers nobody has waited for (an import behind a collective)
    return guarded_rc([&] { finish_flight_locked(); Engine::get().sync_io(); return 0; });
}
int tfhe_hip_stream_sync(void) {
    auto g = recorder_lock();
    return guarded_rc([&] {
        Engine::get().ensure_init();
        finish_flight_locked();
        Engine::get().sync_stream("tfhe_hip_stream_sync");
        return 0;
    });
}
int tfhe_hip_wait_event(void *event, const char *what) {
    if (!event) { set_error("tfhe_hip_wait_event: null event"); return -1; }
    // the deadline and the label are read under the recorder lock (tfhe_hip_set_tuning / tfhe_hip_set_diag_label write them
    // there); the wait itself holds no lock -- it may last until a peer process arrives, and other threads go on recording
    long long deadline_ms;
    std::string label;
    {
        auto g = recorder_lock();
        Engine::get().ensure_init();
        deadline_ms = Engine::get().sync_deadline_ms;
        label = Engine::get().diag_label;
    }
    return guarded_rc([&] {
        Engine::get().wait_event(static_cast<hipEvent_t>(event), what && *what ? what : "tfhe_hip_wait_event", deadline_ms, label);
        return 0;
    });
}
int tfhe_hip_device_pci_bus_id(char *out, int len) {
    if (!out || len < 16) { set_error("tfhe_hip_device_pci_bus_id: buffer of at least 16 bytes needed"); return -1; }
    return guarded_rc([&] {
        Engine::get().ensure_init();
        return Engine::get().pci_bus_id(out, len) ? 0 : -1;
    });
}
void tfhe_hip_set_diag_label(const char *label) {
    auto g = recorder_lock();
    Engine::get().diag_label = label ? std::string(label).substr(0, 127) : std::string();
}

int tfhe_hip_gate_batch(int gate, LweSample *result, const LweSample *a, const LweSample *b, int32_t count,
                        const TFheGateBootstrappingCloudKeySet *bk) {
    if (gate < 0 || gate > TFHE_HIP_ORYN) { set_error("tfhe_hip_gate_batch: bad gate code"); return -1; }
    return record_batch([&] {
        for (int32_t i = 0; i < count; ++i) record_gate2_locked(gate, &result[i], &a[i], &b[i], bk);
    });
}

static bool gate3_args_ok(const char *who, int gate, int negate_mask) {
    if (gate < TFHE_HIP_MAJ3 || gate > TFHE_HIP_XNOR3) { set_error(std::string(who) + ": bad gate code"); return false; }
    if (negate_mask < 0 || negate_mask > 7) { set_error(std::string(who) + ": bad negation mask"); return false; }
    return true;
}

void tfhe_hip_gate3(int gate, int negate_mask, LweSample *result, const LweSample *a, const LweSample *b, const LweSample *c,
                    const TFheGateBootstrappingCloudKeySet *bk) {
    if (!gate3_args_ok("tfhe_hip_gate3", gate, negate_mask)) return;
    guarded([&] {
        auto g = recorder_lock();
        record_gate3_locked(gate, negate_mask, result, a, b, c, bk);
    });
}

int tfhe_hip_gate3_batch(int gate, int negate_mask, LweSample *result, const LweSample *a, const LweSample *b,
                         const LweSample *c, int32_t count, const TFheGateBootstrappingCloudKeySet *bk) {
    if (!gate3_args_ok("tfhe_hip_gate3_batch", gate, negate_mask)) return -1;
    return record_batch([&] {
        for (int32_t i = 0; i < count; ++i) record_gate3_locked(gate, negate_mask, &result[i], &a[i], &b[i], &c[i], bk);
    });
}

// ---- programmable bootstrap: caller-supplied test polynomials ----
}  // extern "C"

// A test polynomial bound to a ring size.  Its words reach the device at first use (a LUT can be built, read and
// deleted on a machine without a GPU); `dev` is then its entry in the engine's table.
struct TfheHipLut {
    uint32_t magic;
    int32_t N;
    std::vector<Torus32> words;
    int32_t dev;
};

namespace {
constexpr uint32_t LUT_MAGIC = 0x4C55547Fu;

TfheHipLut *make_lut(const char *who, const TFheGateBootstrappingParameterSet *params, const Torus32 *v) {
    if (!params || !params->tgsw_params || !params->tgsw_params->tlwe_params) { set_error(std::string(who) + ": null parameter set"); return nullptr; }
    const int32_t N = params->tgsw_params->tlwe_params->N;
    if (N < 1 || N > LUT_STRIDE) { set_error(std::string(who) + ": ring size out of range"); return nullptr; }
    auto *lut = new TfheHipLut{LUT_MAGIC, N, std::vector<Torus32>(), -1};
    if (v) lut->words.assign(v, v + N);
    else lut->words.assign((size_t)N, 0);
    return lut;
}

// the checks every LUT bootstrap makes before anything is recorded; the LUT's entry in the engine's table (uploaded here at
// first use: out of device memory is an ApiError, the call then has no effect)
int32_t lut_entry(const TfheHipLut *lut, int32_t nin, const void *in, const int32_t *coef,
                  const TFheGateBootstrappingCloudKeySet *bk) {
    if (!lut || lut->magic != LUT_MAGIC) api_fail("tfhe_hip_lut_bootstrap: null or deleted LUT");
    if (nin < 1 || nin > 3) api_fail("tfhe_hip_lut_bootstrap: nin must be 1, 2 or 3");
    if (!in || !coef) api_fail("tfhe_hip_lut_bootstrap: null operand or coefficient list");
    if (!bk || !bk->bk) api_fail("null cloud key");
    if (bk->bk->p.N != lut->N)
        api_fail("tfhe_hip_lut_bootstrap: the LUT holds " + std::to_string(lut->N) + " words, the key's ring has " +
                 std::to_string(bk->bk->p.N));
    if (lut->dev < 0) {
        pool_of_key(bk);                                  // (the key image first: what initialises the device)
        const_cast<TfheHipLut *>(lut)->dev = Engine::get().lut_add(lut->words.data(), lut->N);
    }
    return lut->dev;
}
}  // namespace

extern "C" {

TfheHipLut *tfhe_hip_new_lut(const TFheGateBootstrappingParameterSet *params, const Torus32 *v) {
    if (!v) { set_error("tfhe_hip_new_lut: null words"); return nullptr; }
    return make_lut("tfhe_hip_new_lut", params, v);
}

TfheHipLut *tfhe_hip_new_lut_constant(const TFheGateBootstrappingParameterSet *params, Torus32 mu) {
    TfheHipLut *lut = make_lut("tfhe_hip_new_lut_constant", params, nullptr);
    if (lut) std::fill(lut->words.begin(), lut->words.end(), mu);
    return lut;
}

TfheHipLut *tfhe_hip_new_lut_from_table(const TFheGateBootstrappingParameterSet *params, const Torus32 *values, int32_t slots) {
    if (!values) { set_error("tfhe_hip_new_lut_from_table: null values"); return nullptr; }
    TfheHipLut *lut = make_lut("tfhe_hip_new_lut_from_table", params, nullptr);
    if (!lut) return nullptr;
    if (slots < 1 || lut->N % slots != 0) {
        set_error("tfhe_hip_new_lut_from_table: slots must divide N = " + std::to_string(lut->N));
        delete lut;
        return nullptr;
    }
    for (int32_t j = 0; j < lut->N; ++j) lut->words[(size_t)j] = values[(int64_t)j * slots / lut->N];
    return lut;
}

void tfhe_hip_delete_lut(TfheHipLut *lut) {
    if (!lut) return;
    if (lut->magic != LUT_MAGIC) { set_error("tfhe_hip_delete_lut: not a LUT (or already deleted)"); return; }
    auto g = recorder_lock();
    if (lut->dev >= 0) {
        guarded([&] { forget_lut_locked(lut->dev); });    // recorded ops that name it run first, as for a key
        Engine::get().lut_free(lut->dev);
    }
    lut->magic = 0;
    delete lut;
}

const Torus32 *tfhe_hip_lut_words(const TfheHipLut *lut, int32_t *count) {
    if (!lut || lut->magic != LUT_MAGIC) { set_error("tfhe_hip_lut_words: null or deleted LUT"); if (count) *count = 0; return nullptr; }
    if (count) *count = lut->N;
    return lut->words.data();
}

void tfhe_hip_lut_bootstrap(const TfheHipLut *lut, LweSample *result, int32_t nin, const LweSample *const *in,
                            const int32_t *coef, Torus32 c0, const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        const int32_t entry = lut_entry(lut, nin, in, coef, bk);
        record_lut_locked(entry, result, nin, in, coef, c0, bk);
    });
}

int tfhe_hip_lut_bootstrap_batch(const TfheHipLut *lut, LweSample *result, int32_t nin, const LweSample *const *in,
                                 const int32_t *coef, Torus32 c0, int32_t count, const TFheGateBootstrappingCloudKeySet *bk) {
    return record_batch([&] {
        const int32_t entry = lut_entry(lut, nin, in, coef, bk);
        for (int32_t i = 0; i < count; ++i) {
            const LweSample *ops[3] = {&in[0][i], nin > 1 ? &in[1][i] : nullptr, nin > 2 ? &in[2][i] : nullptr};
            record_lut_locked(entry, &result[i], nin, ops, coef, c0, bk);
        }
    });
}

// ---- multi-output programmable bootstrap: several extractions from one rotation ----
}  // extern "C"

// A test polynomial (the object's own copy of the LUT's words, with an entry of its own in the engine's table) and an
// extract spec.  Both reach the device at first use.
struct TfheHipLutMulti {
    uint32_t magic;
    TfheHipLut lut;
    ExtractSpec spec;
    int32_t dev_spec;
};

namespace {
constexpr uint32_t LUTM_MAGIC = 0x4C554D7Fu;

TfheHipLutMulti *make_lut_multi(const char *who, int32_t N, const Torus32 *words, const ExtractSpec &xs) {
    if (const char *why = extract_spec_error(xs, N)) { set_error(std::string(who) + ": " + why); return nullptr; }
    auto *mo = new TfheHipLutMulti{LUTM_MAGIC, TfheHipLut{LUT_MAGIC, N, std::vector<Torus32>(words, words + N), -1}, xs, -1};
    return mo;
}

// the checks every multi-output bootstrap makes before anything is recorded (the LUT entry's, then the results');
// both table entries are uploaded here at first use
void lutm_entry(const TfheHipLutMulti *mo, int32_t nin, const void *in, const int32_t *coef,
                const TFheGateBootstrappingCloudKeySet *bk) {
    if (!mo || mo->magic != LUTM_MAGIC) api_fail("tfhe_hip_lut_bootstrap_multi: null or deleted multi-output LUT");
    lut_entry(&mo->lut, nin, in, coef, bk);
    if (mo->dev_spec < 0) const_cast<TfheHipLutMulti *>(mo)->dev_spec = Engine::get().spec_add(mo->spec);
}
void lutm_check_results(const TfheHipLutMulti *mo, LweSample *const *result) {
    if (!mo || mo->magic != LUTM_MAGIC) api_fail("tfhe_hip_lut_bootstrap_multi: null or deleted multi-output LUT");
    if (!result) api_fail("tfhe_hip_lut_bootstrap_multi: null result list");
    bool any = false;
    for (int m = 0; m < mo->spec.nout; ++m) {
        any |= result[m] != nullptr;
        for (int o = 0; o < m; ++o)
            if (result[m] && result[m] == result[o]) api_fail("tfhe_hip_lut_bootstrap_multi: two results are the same sample");
    }
    if (!any) api_fail("tfhe_hip_lut_bootstrap_multi: every result is null");
}
}  // namespace

extern "C" {

TfheHipLutMulti *tfhe_hip_new_lut_multi(const TfheHipLut *lut, int32_t nout, const int32_t *ntaps, const int32_t *tap_index,
                                        const int32_t *tap_weight, const Torus32 *out_c0) {
    const char *who = "tfhe_hip_new_lut_multi";
    if (!lut || lut->magic != LUT_MAGIC) { set_error(std::string(who) + ": null or deleted LUT"); return nullptr; }
    if (!ntaps || !tap_index || !tap_weight) { set_error(std::string(who) + ": null tap list"); return nullptr; }
    if (nout < 1 || nout > XS_MAX_OUT) { set_error(std::string(who) + ": nout must be 1..4"); return nullptr; }
    ExtractSpec xs{};
    xs.nout = nout;
    size_t at = 0;
    for (int m = 0; m < nout; ++m) {
        if (ntaps[m] < 1 || ntaps[m] > XS_MAX_TAPS) { set_error(std::string(who) + ": an output takes 1..8 taps"); return nullptr; }
        xs.ntaps[m] = ntaps[m];
        xs.out_c0[m] = out_c0 ? out_c0[m] : 0;
        for (int t = 0; t < ntaps[m]; ++t, ++at) { xs.index[m][t] = tap_index[at]; xs.weight[m][t] = tap_weight[at]; }
    }
    return make_lut_multi(who, lut->N, lut->words.data(), xs);
}

TfheHipLutMulti *tfhe_hip_new_lut_multi_from_tables(const TFheGateBootstrappingParameterSet *params, Torus32 step, int32_t slots,
                                                    int32_t nout, const int32_t *levels) {
    const char *who = "tfhe_hip_new_lut_multi_from_tables";
    if (!params || !params->tgsw_params || !params->tgsw_params->tlwe_params) { set_error(std::string(who) + ": null parameter set"); return nullptr; }
    const int32_t N = params->tgsw_params->tlwe_params->N;
    if (N < 1 || N > LUT_STRIDE) { set_error(std::string(who) + ": ring size out of range"); return nullptr; }
    if (!levels) { set_error(std::string(who) + ": null levels"); return nullptr; }
    if (step & 1) { set_error(std::string(who) + ": step must be even (the test polynomial is the constant step/2)"); return nullptr; }
    if (slots < 2 || N % slots != 0) { set_error(std::string(who) + ": slots must be at least 2 and divide N = " + std::to_string(N)); return nullptr; }
    if (nout < 1 || nout > XS_MAX_OUT) { set_error(std::string(who) + ": nout must be 1..4"); return nullptr; }
    // Coefficient j N/slots of X^-p (step/2) decrypts to +step/2 for p in a sector s <= slots-1-j and to -step/2 above:
    // with weights L[slots-1-j] - L[slots-j] the taps sum to step L[s] - (step/2)(L[0] + L[slots-1]) (include/tfhe_hip.h)
    ExtractSpec xs{};
    xs.nout = nout;
    const uint32_t half = (uint32_t)(step / 2);
    for (int m = 0; m < nout; ++m) {
        const int32_t *L = levels + (size_t)m * slots;
        int nt = 0;
        for (int j = 1; j < slots; ++j) {
            const int64_t w = (int64_t)L[slots - 1 - j] - (int64_t)L[slots - j];
            if (w == 0) continue;
            if (w > XS_MAX_WEIGHT || w < -XS_MAX_WEIGHT) { set_error(std::string(who) + ": neighbouring levels differ by more than 8"); return nullptr; }
            if (nt == XS_MAX_TAPS) { set_error(std::string(who) + ": an output would need more than 8 taps"); return nullptr; }
            xs.index[m][nt] = j * (N / slots);
            xs.weight[m][nt] = (int32_t)w;
            ++nt;
        }
        if (nt == 0) { set_error(std::string(who) + ": an output with equal levels in every sector needs no tap (it is a constant)"); return nullptr; }
        xs.ntaps[m] = nt;
        xs.out_c0[m] = (int32_t)(half * ((uint32_t)L[0] + (uint32_t)L[slots - 1]));
    }
    const std::vector<Torus32> words((size_t)N, (Torus32)half);
    return make_lut_multi(who, N, words.data(), xs);
}

void tfhe_hip_delete_lut_multi(TfheHipLutMulti *mo) {
    if (!mo) return;
    if (mo->magic != LUTM_MAGIC) { set_error("tfhe_hip_delete_lut_multi: not a multi-output LUT (or already deleted)"); return; }
    auto g = recorder_lock();
    if (mo->lut.dev >= 0 || mo->dev_spec >= 0) {
        guarded([&] { forget_lutm_locked(mo->lut.dev, mo->dev_spec); });    // recorded ops that name it run first
        if (mo->lut.dev >= 0) Engine::get().lut_free(mo->lut.dev);
        if (mo->dev_spec >= 0) Engine::get().spec_free(mo->dev_spec);
    }
    mo->magic = 0;
    mo->lut.magic = 0;
    delete mo;
}

int32_t tfhe_hip_lut_multi_nout(const TfheHipLutMulti *mo) {
    if (!mo || mo->magic != LUTM_MAGIC) { set_error("tfhe_hip_lut_multi_nout: null or deleted multi-output LUT"); return -1; }
    return mo->spec.nout;
}

int32_t tfhe_hip_lut_multi_output(const TfheHipLutMulti *mo, int32_t m, int32_t *tap_index, int32_t *tap_weight, Torus32 *out_c0) {
    if (!mo || mo->magic != LUTM_MAGIC) { set_error("tfhe_hip_lut_multi_output: null or deleted multi-output LUT"); return -1; }
    if (m < 0 || m >= mo->spec.nout) { set_error("tfhe_hip_lut_multi_output: no such output"); return -1; }
    for (int t = 0; t < mo->spec.ntaps[m]; ++t) {
        if (tap_index) tap_index[t] = mo->spec.index[m][t];
        if (tap_weight) tap_weight[t] = mo->spec.weight[m][t];
    }
    if (out_c0) *out_c0 = mo->spec.out_c0[m];
    return mo->spec.ntaps[m];
}

const Torus32 *tfhe_hip_lut_multi_words(const TfheHipLutMulti *mo, int32_t *count) {
    if (!mo || mo->magic != LUTM_MAGIC) { set_error("tfhe_hip_lut_multi_words: null or deleted multi-output LUT"); if (count) *count = 0; return nullptr; }
    if (count) *count = mo->lut.N;
    return mo->lut.words.data();
}

void tfhe_hip_lut_bootstrap_multi(const TfheHipLutMulti *mo, LweSample *const *result, int32_t nin, const LweSample *const *in,
                                  const int32_t *coef, Torus32 c0, const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        lutm_check_results(mo, result);
        lutm_entry(mo, nin, in, coef, bk);
        record_lutm_locked(mo->lut.dev, mo->dev_spec, mo->spec.nout, result, nin, in, coef, c0, bk);
    });
}

int tfhe_hip_lut_bootstrap_multi_batch(const TfheHipLutMulti *mo, LweSample *const *result, int32_t nin,
                                       const LweSample *const *in, const int32_t *coef, Torus32 c0, int32_t count,
                                       const TFheGateBootstrappingCloudKeySet *bk) {
    return record_batch([&] {
        lutm_check_results(mo, result);
        lutm_entry(mo, nin, in, coef, bk);
        for (int32_t i = 0; i < count; ++i) {
            const LweSample *ops[3] = {&in[0][i], nin > 1 ? &in[1][i] : nullptr, nin > 2 ? &in[2][i] : nullptr};
            LweSample *res[XS_MAX_OUT] = {nullptr, nullptr, nullptr, nullptr};
            for (int m = 0; m < mo->spec.nout; ++m) res[m] = result[m] ? &result[m][i] : nullptr;
            record_lutm_locked(mo->lut.dev, mo->dev_spec, mo->spec.nout, res, nin, ops, coef, c0, bk);
        }
    });
}

// ---- linear combinations of samples: no bootstrap, no key switch ----
static void linear_args_check(const char *who, const void *result, int32_t nin, const void *in, const int32_t *coef,
                              const TFheGateBootstrappingCloudKeySet *bk) {
    if (nin < 1 || nin > TFHE_HIP_LINEAR_MAX_IN) api_fail(std::string(who) + ": nin must be 1..16");
    if (!result) api_fail(std::string(who) + ": null result");
    if (!in || !coef) api_fail(std::string(who) + ": null operand or coefficient list");
    for (int32_t i = 0; i < nin; ++i)
        if (!static_cast<const void *const *>(in)[i]) api_fail(std::string(who) + ": null operand");
    if (!bk || !bk->bk) api_fail("null cloud key");
}
// a sample of the call, before the key is touched: ours, and of the key's LWE dimension
static void linear_sample_check(const LweSample *s, const TFheGateBootstrappingCloudKeySet *bk) {
    if (header_of(s)->n != bk->bk->p.n) api_fail("ciphertext used with a key of different LWE dimension than the one it was allocated for");
}

void tfhe_hip_linear(LweSample *result, int32_t nin, const LweSample *const *in, const int32_t *coef, Torus32 c0,
                     const TFheGateBootstrappingCloudKeySet *bk) {
    static_assert(TFHE_HIP_LINEAR_MAX_IN == LIN_MAX_IN && LIN_MAX_IN == LIN_DESC_MAX_IN, "one limit, from the header to the kernel");
    guarded([&] {
        linear_args_check("tfhe_hip_linear", result, nin, in, coef, bk);
        linear_sample_check(result, bk);
        for (int32_t i = 0; i < nin; ++i) linear_sample_check(in[i], bk);
        auto g = recorder_lock();
        record_linear_locked(result, nin, in, coef, c0, bk);
    });
}

int tfhe_hip_linear_batch(LweSample *result, int32_t nin, const LweSample *const *in, const int32_t *coef, Torus32 c0,
                          int32_t count, const TFheGateBootstrappingCloudKeySet *bk) {
    auto g = recorder_lock();
    const int rc = record_batch([&] {
        linear_args_check("tfhe_hip_linear_batch", result, nin, in, coef, bk);
        if (count > 0) {
            linear_sample_check(result, bk);
            for (int32_t k = 0; k < nin; ++k) linear_sample_check(in[k], bk);
        }
        for (int32_t i = 0; i < count; ++i) {
            const LweSample *ops[LIN_MAX_IN];
            for (int32_t k = 0; k < nin; ++k) ops[k] = &in[k][i];
            record_linear_locked(&result[i], nin, ops, coef, c0, bk);
        }
    });
    // immediate mode: complete on return, host mirrors refreshed like tfhe_hip_linear's
    if (rc == 0 && !deferred_mode())
        return guarded_rc([&] { for (int32_t i = 0; i < count; ++i) sync_sample_locked(&result[i]); return 0; });
    return rc;
}

void tfhe_hip_test_set_alloc_cap(int64_t bytes) {
    auto g = recorder_lock();
    set_alloc_cap((long long)bytes);
}

int tfhe_hip_test_stage_place(int64_t pos, int64_t capacity, int32_t outstanding, int64_t bytes, int64_t *out4) {
    if (pos < 0 || capacity < 0 || bytes < 0 || !out4) { set_error("test_stage_place: bad arguments"); return -1; }
    const StagePlace p = stage_place((size_t)pos, (size_t)capacity, outstanding != 0, (size_t)bytes);
    out4[0] = (int64_t)p.offset; out4[1] = p.wait ? 1 : 0; out4[2] = (int64_t)p.capacity; out4[3] = (int64_t)p.next;
    return 0;
}

int tfhe_hip_test_form_admissible(int form, int32_t N, int32_t l, int32_t Bgbit, int tables) {
    return br_form_admissible(form, N, l, Bgbit, tables) ? 1 : 0;
}

int tfhe_hip_set_tuning(const char *name, int64_t value) {
    auto g = recorder_lock();      // the launchers read the tunings under the same lock (flushes)
    if (name && std::strcmp(name, "ks_tile") == 0) {
        if (value != 0 && value != 16 && value != 24 && value != 32) { set_error("ks_tile must be 0, 16, 24 or 32"); return -1; }
        Engine::get().tunings.ks_tile = (int)value;
        return 0;
    }
    if (name && std::strcmp(name, "ks_index") == 0) { Engine::get().tunings.ks_index = value != 0; return 0; }
    if (name && std::strcmp(name, "ks_max_splits") == 0) {
        if (value < 1 || value > 64) { set_error("ks_max_splits must be in [1, 64]"); return -1; }
        Engine::get().tunings.ks_max_splits = (int)value;
        return 0;
    }
    if (name && std::strcmp(name, "br_digit_table") == 0) { Engine::get().tunings.br_digit_table = (int)value; return 0; }
    if (name && std::strcmp(name, "br8_max_rotations") == 0) { Engine::get().tunings.br8_max_rotations = (int)value; return 0; }
    if (name && std::strcmp(name, "br_tail8") == 0) { Engine::get().tunings.br_tail8 = (int)value; return 0; }
    if (name && std::strcmp(name, "br_variant") == 0) { Engine::get().tunings.br_variant = (int)value; return 0; }
    if (name && set_recorder_tuning_locked(name, value != 0)) return 0;   // reuse_gates, eliminate_dead, fold_constants, balance_levels, batch_keys, level_slack
    if (name && std::strcmp(name, "sync_deadline_ms") == 0) { Engine::get().sync_deadline_ms = value > 0 ? (long long)value : 0; return 0; }
    set_error(std::string("tfhe_hip_set_tuning: unknown name ") + (name ? name : "(null)"));
    return -1;
}

// the statistics are only ever written under the recorder lock (flushes, reuse counters, test paths)
void tfhe_hip_get_stats(TfheHipStats *out) {
    auto g = recorder_lock();
    Engine::get().wait_flight();          // the times of an asynchronous flush are read when it has completed
    if (out) *out = Engine::get().stats;
}
void tfhe_hip_reset_stats(void) {
    auto g = recorder_lock();
    Engine::get().stats = TfheHipStats{};
    Engine::get().expand_stats = TfheHipExpandStats{};
    Engine::get().seeded_stats = TfheHipSeededStats{};
    Engine::get().seeded_lwe_stats = TfheHipSeededLweStats{};
}
void tfhe_hip_get_seeded_stats(TfheHipSeededStats *out) {
    auto g = recorder_lock();
    if (out) *out = Engine::get().seeded_stats;
}
void tfhe_hip_get_expand_stats(TfheHipExpandStats *out) {
    auto g = recorder_lock();
    if (out) *out = Engine::get().expand_stats;
}
void tfhe_hip_set_kernel_timing(int on) { Engine::get().kernel_timing = on != 0; }
int tfhe_hip_last_flush_keys(void) {
    auto g = recorder_lock();
    return Engine::get().last_flush_keys;
}
int tfhe_hip_set_batch_keys(int on) {
    auto g = recorder_lock();
    return set_batch_keys_locked(on != 0) ? 1 : 0;
}

static int test_build_ops(const int32_t *ops5, int32_t count, std::vector<PendingOp> &ops) {
    // ops5[i] = {kind, dst, a, b, c}; ASAP levels are derived here exactly as the recorder derives them
    for (int32_t i = 0; i < count; ++i)
        if (!op_kind_valid(ops5[5 * (size_t)i])) { set_error("test schedule: unknown op kind"); return -1; }
    ops.resize((size_t)count);
    std::vector<int32_t> slot_level;
    int depth = 0;
    auto level_of = [&](int32_t s) { return s >= 0 && (size_t)s < slot_level.size() ? slot_level[s] : 0; };
    for (int32_t i = 0; i < count; ++i) {
        const int32_t *o = ops5 + 5 * (size_t)i;
        PendingOp op{(uint8_t)o[0], o[1], o[2], o[3], o[4], 0};
        const int32_t in = std::max(level_of(op.a), std::max(level_of(op.b), level_of(op.c)));
        op.level = op.kind == OP_NOT ? in : in + 1;
        if ((size_t)op.dst >= slot_level.size()) slot_level.resize((size_t)op.dst + 1, 0);
        slot_level[op.dst] = op.level;
        depth = std::max(depth, op.level);
        ops[i] = op;
    }
    return depth;
}

int tfhe_hip_test_schedule(const int32_t *ops5, int32_t count, int32_t unit, int32_t balance, int32_t *levels_out) {
    std::vector<PendingOp> ops;
    const int depth = test_build_ops(ops5, count, ops);
    if (depth < 0) return -1;
    std::vector<int32_t> lvl;
    const int d = schedule_levels(ops, depth, balance != 0, unit, lvl);
    for (int32_t i = 0; i < count; ++i) levels_out[i] = lvl[i];
    return d;
}

int tfhe_hip_test_level_slack(const int32_t *ops5, int32_t count, int32_t unit, int32_t level_slack, const int32_t *cost_widths,
                              const double *cost_us, int32_t ncost, int32_t period, int32_t *levels_out, int32_t *widths_out,
                              double *cost_out2) {
    if (!ops5 || count < 0 || unit < 1 || ncost < 0 || period < 0 || (ncost > 0 && (!cost_widths || !cost_us)) || !levels_out || !widths_out ||
        !cost_out2) {
        set_error("test_level_slack: bad arguments");
        return -1;
    }
    for (int32_t j = 0; j < ncost; ++j)
        if (cost_widths[j] < 1 || (j > 0 && cost_widths[j] <= cost_widths[j - 1]) || !(cost_us[j] >= 0)) {
            set_error("test_level_slack: the table's widths must ascend from 1 on, its costs must not be negative");
            return -1;
        }
    std::vector<PendingOp> ops;
    const int depth = test_build_ops(ops5, count, ops);
    if (depth < 0) return -1;
    std::vector<int32_t> lvl;
    const LevelCost table{cost_widths, cost_us, ncost, period}, none;
    LevelSlackReport report;
    schedule_levels(ops, depth, true, unit, lvl, nullptr, nullptr, level_slack ? &table : &none, &report);
    std::fill(widths_out, widths_out + depth + 1, 0);
    for (int32_t i = 0; i < count; ++i) {
        levels_out[i] = lvl[i];
        widths_out[lvl[i]] += op_rotations(ops[i]);
    }
    cost_out2[0] = cost_out2[1] = 0;
    for (int L = 1; L <= depth; ++L) cost_out2[0] += level_cost_at(table, widths_out[L]);
    // the sum without the pass: the pass reports it when it ran, else the levels are those
    cost_out2[1] = report.moved ? report.us_before : cost_out2[0];
    return depth;
}

int tfhe_hip_test_level_cost(int32_t n, int32_t N, int32_t k, int32_t l, int32_t Bgbit, int32_t ks_t, int32_t ks_basebit,
                             int32_t cu_count, int32_t width, double *us_out) {
    if (!us_out) { set_error("test_level_cost: null output"); return -1; }
    *us_out = level_cost_us(width, LevelCostSet{n, N, k, l, Bgbit, ks_t, ks_basebit}, cu_count, LaunchTunings{});
    return 0;
}

int tfhe_hip_test_set_level_cost(const int32_t *cost_widths, const double *cost_us, int32_t ncost) {
    if (ncost < 0 || (ncost > 0 && (!cost_widths || !cost_us))) { set_error("test_set_level_cost: bad arguments"); return -1; }
    for (int32_t j = 0; j < ncost; ++j)
        if (cost_widths[j] < 1 || (j > 0 && cost_widths[j] <= cost_widths[j - 1]) || !(cost_us[j] >= 0)) {
            set_error("test_set_level_cost: the table's widths must ascend from 1 on, its costs must not be negative");
            return -1;
        }
    auto g = recorder_lock();
    set_level_cost_locked(cost_widths, cost_us, ncost);
    return 0;
}

int tfhe_hip_last_level_slack(double *out4) {
    if (!out4) { set_error("last_level_slack: null output"); return -1; }
    auto g = recorder_lock();
    last_level_slack_locked(out4);
    return 0;
}

// rot_words = 6: the two-operand words of every rotation (the form older callers know); 8: slot_c and sc as well; 9: and
// the LUT index; 10: and the extract spec word.  ops = ops5, or records of 10 words when lut_ops
// (tfhe_hip_test_level_plan_lut), or of 16 when rec_words = 16 (tfhe_hip_test_level_plan_multi: dead_slots as well).
// lin (tfhe_hip_test_level_plan_lin): records of kind 66 name terms of lin->terms2; their part of the plan goes to lin->*
// (tfhe_hip_test_level_plan_full: lin->not_off and lin->nots2 are set and receive LevelPlan::not_off / nots)
struct TestLinPlan {
    const int32_t *terms2; int32_t nterms;
    int32_t *ranks_out, *sizes2, *level_off, *launch_off, *launch_rank, *descs35;
    int32_t *not_off = nullptr, *nots2 = nullptr;            // tfhe_hip_test_level_plan_full: the NOT descriptors as well
};
static int test_level_plan(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                           int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                           int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots, int rot_words, int32_t *kss4,
                           bool lut_ops = false, int32_t reuse = 0, int32_t *shared_with = nullptr, int rec_words = 10,
                           const int32_t *dead_slots = nullptr, int32_t ndead = 0, const TestLinPlan *lin = nullptr) {
    if (count < 0 || nkeys < 1 || nkeys > UINT16_MAX) { set_error("test_level_plan: bad count or nkeys"); return -1; }
    for (int32_t i = 0; i < count; ++i)
        if (op_keys[i] < 0 || op_keys[i] >= nkeys) { set_error("test_level_plan: key index out of range"); return -1; }
    std::vector<PendingOp> ops;
    std::vector<int32_t> op_of_record;                   // lut_ops: record -> index in ops (-1: eliminated)
    std::vector<LinTerm> terms;                          // the graph's term table (records of kind 66)
    int depth;
    if (!lut_ops) {
        depth = test_build_ops(ops5, count, ops);
        if (depth < 0) return -1;
        for (int32_t i = 0; i < count; ++i) ops[i].key = (uint16_t)op_keys[i];
    } else {
        // The records go through the recorder's own graph (op_graph.hpp) over a plain slot table.  Every id of the records
        // is a handle that holds the slot of its own number; the destination ids of a record are the fresh slots the graph
        // is offered, and a record that was shared re-points its handles, so later records read what the recorder's
        // would.  shared_with[i] = the record whose op record i shares or widens, or -1.
        struct SlotTable {
            std::vector<int32_t> ref, level;
            std::vector<uint8_t> pending;
            void retain(int32_t s) { ++ref[(size_t)s]; }
            void release(int32_t s) { --ref[(size_t)s]; }
            int32_t refs(int32_t s) const { return ref[(size_t)s]; }
        };
        const int id_words = rec_words == 16 ? 4 : 0;            // the destinations of a multi-output record: words 12..15
        int32_t top = 0;
        for (int32_t i = 0; i < count; ++i) {
            const int32_t *o = ops5 + (size_t)rec_words * (size_t)i;
            for (int w = 1; w <= 4; ++w) top = std::max(top, o[w] + 1);
            for (int w = 12; w < 12 + id_words; ++w) top = std::max(top, o[w] + 1);
            if (lin && o[0] == OP_LIN) {
                if (o[5] < 0 || o[6] < 1 || o[6] > LIN_MAX_IN || o[5] > lin->nterms - o[6]) { set_error("test_level_plan_lin: bad term range"); return -1; }
                for (int t = 0; t < o[6]; ++t) {
                    if (lin->terms2[2 * (size_t)(o[5] + t)] < 0) { set_error("test_level_plan_lin: a term without an operand"); return -1; }
                    top = std::max(top, lin->terms2[2 * (size_t)(o[5] + t)] + 1);
                }
            }
        }
        SlotTable slots{std::vector<int32_t>((size_t)top, 1), std::vector<int32_t>((size_t)top, 0), std::vector<uint8_t>((size_t)top, 0)};
        std::vector<int32_t> handle((size_t)top), record_of_op;
        std::iota(handle.begin(), handle.end(), 0);
        OpGraph<SlotTable> graph;
        graph.reuse = reuse != 0;
        op_of_record.assign((size_t)count, -1);
        for (int32_t i = 0; i < count; ++i) {
            const int32_t *o = ops5 + (size_t)rec_words * (size_t)i;
            const bool multi = rec_words == 16 && o[0] == OP_LUTM;
            const bool is_lin = lin && o[0] == OP_LIN;
            if (!op_kind_valid_lut(o[0]) && !multi && !is_lin) { set_error("test schedule: unknown op kind"); return -1; }
            auto slot_of = [&](int32_t id) { return id >= 0 ? handle[(size_t)id] : -1; };
            PendingOp op{(uint8_t)o[0], -1, slot_of(o[2]), slot_of(o[3]), slot_of(o[4]), 0, (uint16_t)op_keys[i]};
            if (op.kind == OP_LUT || multi) { op.lut = o[5]; op.sa = o[6]; op.sb = o[7]; op.sc = o[8]; op.c0 = o[9]; }
            int32_t ids[4] = {o[1], -1, -1, -1}, out[4];
            if (multi) {
                op.spec = o[10]; op.nout = o[11];
                if (op.nout < 1 || op.nout > XS_MAX_OUT) { set_error("test_level_plan_multi: nout must be 1..4"); return -1; }
                std::copy(o + 12, o + 12 + op.nout, ids);
            }
            LinTerm lt[LIN_MAX_IN];
            if (is_lin) {
                op.a = op.b = op.c = -1;
                op.nout = o[6]; op.c0 = o[9];
                for (int t = 0; t < op.nout; ++t) lt[t] = LinTerm{slot_of(lin->terms2[2 * (size_t)(o[5] + t)]), lin->terms2[2 * (size_t)(o[5] + t) + 1]};
            }
            unsigned wanted = 0;
            for (int m = 0; m < op_outputs(op); ++m) {
                if (ids[m] < 0) continue;
                if (handle[(size_t)ids[m]] != ids[m] || slots.pending[(size_t)ids[m]] || std::count(ids, ids + m, ids[m])) {
                    set_error("test_level_plan: a destination id used twice");
                    return -1;
                }
                wanted |= 1u << m;
            }
            if (!wanted) { set_error("test_level_plan: an op without a destination"); return -1; }
            const int32_t shared = graph.record(slots, op, wanted, [&](int m) { return ids[m]; }, out, is_lin ? lt : nullptr);
            if (shared < 0) record_of_op.push_back(i);
            if (shared_with) shared_with[i] = shared < 0 ? -1 : record_of_op[(size_t)shared];
            op_of_record[(size_t)i] = shared < 0 ? (int32_t)record_of_op.size() - 1 : shared;
            for (int m = 0; m < op_outputs(op); ++m)
                if ((wanted >> m & 1) && out[m] != ids[m]) { slots.release(ids[m]); handle[(size_t)ids[m]] = out[m]; }   // (recorder.cpp repoint)
        }
        for (int32_t d = 0; d < ndead; ++d) {                    // these handles are gone before the flush
            const int32_t id = dead_slots[d];
            if (id < 0 || id >= top || handle[(size_t)id] < 0) continue;
            slots.release(handle[(size_t)id]);
            handle[(size_t)id] = -1;
        }
        std::vector<int32_t> moved_to;
        graph.eliminate_dead(slots, &moved_to);
        for (int32_t &at : op_of_record) at = moved_to[(size_t)at];
        ops = graph.ops();
        terms.assign(graph.terms(), graph.terms() + graph.term_count());
        depth = graph.max_level();
    }
    std::vector<int32_t> lvl;
    const int levels = schedule_levels(ops, depth, balance != 0, unit, lvl, nullptr, terms.data());
    const LevelPlan plan = build_level_plan(ops, lvl, levels, nkeys, terms.data());     // exactly what flush_locked hands to execute()
    for (int32_t i = 0; i < count; ++i) {
        const int32_t at = lut_ops ? op_of_record[(size_t)i] : i;
        levels_out[i] = at >= 0 ? lvl[(size_t)at] : -1;      // -1: eliminated (tfhe_hip_test_level_plan_multi's dead_slots)
        if (lin) lin->ranks_out[i] = at < 0 ? -1 : plan.op_rank.empty() ? 0 : plan.op_rank[(size_t)at];
    }
    if (lin) {
        static_assert(sizeof(LinDesc) == 35 * sizeof(int32_t), "a linear descriptor is 35 plain words");
        lin->sizes2[0] = plan.lins.empty() ? 0 : (int32_t)plan.lin_launch_off.size() - 1;
        lin->sizes2[1] = (int32_t)plan.lins.size();
        for (size_t L = 0; L < (size_t)levels + 2; ++L) lin->level_off[L] = plan.lins.empty() ? 0 : plan.lin_level_off[L];
        if (!plan.lins.empty()) {
            std::memcpy(lin->launch_off, plan.lin_launch_off.data(), plan.lin_launch_off.size() * sizeof(int32_t));
            std::memcpy(lin->launch_rank, plan.lin_launch_rank.data(), plan.lin_launch_rank.size() * sizeof(int32_t));
            std::memcpy(lin->descs35, plan.lins.data(), plan.lins.size() * sizeof(LinDesc));
        }
        if (lin->not_off) {
            static_assert(sizeof(NotDesc) == 2 * sizeof(int32_t), "a NOT descriptor is two plain words");
            std::memcpy(lin->not_off, plan.not_off.data(), plan.not_off.size() * sizeof(int32_t));
            if (!plan.nots.empty()) std::memcpy(lin->nots2, plan.nots.data(), plan.nots.size() * sizeof(NotDesc));
        }
    }
    sizes6[0] = plan.levels;
    sizes6[1] = (int32_t)plan.rots.size();
    sizes6[2] = (int32_t)plan.kss.size();
    sizes6[3] = (int32_t)plan.rot_koff.size();
    sizes6[4] = (int32_t)plan.ks_koff.size();
    sizes6[5] = (int32_t)plan.rot_key.size();
    static_assert(sizeof(RotDesc) == 10 * sizeof(int32_t) && offsetof(RotDesc, slot_c) == 6 * sizeof(int32_t) &&
                      offsetof(RotDesc, lut) == 8 * sizeof(int32_t) && offsetof(RotDesc, spec) == 9 * sizeof(int32_t) &&
                      sizeof(KsDesc) == 4 * sizeof(int32_t),
                  "descriptors are plain words: the third operand behind the first six, then the LUT index, the extract spec last");
    auto copy = [](int32_t *dst, const void *src, size_t words) { if (words) std::memcpy(dst, src, words * sizeof(int32_t)); };
    copy(rot_off, plan.rot_off.data(), plan.rot_off.size());
    copy(ks_off, plan.ks_off.data(), plan.ks_off.size());
    copy(rot_koff, plan.rot_koff.data(), plan.rot_koff.size());
    copy(ks_koff, plan.ks_koff.data(), plan.ks_koff.size());
    copy(rot_key, plan.rot_key.data(), plan.rot_key.size());
    for (size_t r = 0; r < plan.rots.size(); ++r) copy(rots + (size_t)rot_words * r, &plan.rots[r], (size_t)rot_words);
    copy(kss4, plan.kss.data(), 4 * plan.kss.size());
    return levels;
}

int tfhe_hip_test_level_plan(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                             int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                             int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots6, int32_t *kss4) {
    return test_level_plan(ops5, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots6, 6, kss4);
}
int tfhe_hip_test_level_plan3(const int32_t *ops5, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                              int32_t balance, int32_t *levels_out, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                              int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots8, int32_t *kss4) {
    return test_level_plan(ops5, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots8, 8, kss4);
}

int tfhe_hip_test_level_plan_lut(const int32_t *ops10, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                 int32_t balance, int32_t reuse, int32_t *levels_out, int32_t *shared_with, int32_t *sizes6,
                                 int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key,
                                 int32_t *rots9, int32_t *kss4) {
    if (reuse && !shared_with) { set_error("test_level_plan_lut: reuse needs shared_with"); return -1; }
    return test_level_plan(ops10, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots9, 9, kss4, true, reuse, shared_with);
}

int tfhe_hip_test_level_plan_multi(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                   int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                   int32_t *levels_out, int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off,
                                   int32_t *rot_koff, int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4) {
    if (!shared_with) { set_error("test_level_plan_multi: shared_with is needed"); return -1; }
    if (ndead < 0 || (ndead > 0 && !dead_slots)) { set_error("test_level_plan_multi: bad dead_slots"); return -1; }
    return test_level_plan(ops16, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots10, 10, kss4, true, reuse, shared_with, 16, dead_slots, ndead);
}

int tfhe_hip_test_level_plan_lin(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                 int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                 const int32_t *lin_terms2, int32_t nterms, int32_t *levels_out, int32_t *ranks_out,
                                 int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff,
                                 int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4, int32_t *lin_sizes2,
                                 int32_t *lin_level_off, int32_t *lin_launch_off, int32_t *lin_launch_rank, int32_t *lins35) {
    if (!shared_with || !ranks_out || !lin_sizes2 || !lin_level_off || !lin_launch_off || !lin_launch_rank || !lins35) {
        set_error("test_level_plan_lin: null output");
        return -1;
    }
    if (ndead < 0 || (ndead > 0 && !dead_slots)) { set_error("test_level_plan_lin: bad dead_slots"); return -1; }
    if (nterms < 0 || (nterms > 0 && !lin_terms2)) { set_error("test_level_plan_lin: bad term table"); return -1; }
    const TestLinPlan lin{lin_terms2, nterms, ranks_out, lin_sizes2, lin_level_off, lin_launch_off, lin_launch_rank, lins35};
    return test_level_plan(ops16, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots10, 10, kss4, true, reuse, shared_with, 16, dead_slots, ndead, &lin);
}

int tfhe_hip_test_level_plan_full(const int32_t *ops16, const int32_t *op_keys, int32_t count, int32_t nkeys, int32_t unit,
                                  int32_t balance, int32_t reuse, const int32_t *dead_slots, int32_t ndead,
                                  const int32_t *lin_terms2, int32_t nterms, int32_t *levels_out, int32_t *ranks_out,
                                  int32_t *shared_with, int32_t *sizes6, int32_t *rot_off, int32_t *ks_off, int32_t *rot_koff,
                                  int32_t *ks_koff, int32_t *rot_key, int32_t *rots10, int32_t *kss4, int32_t *lin_sizes2,
                                  int32_t *lin_level_off, int32_t *lin_launch_off, int32_t *lin_launch_rank, int32_t *lins35,
                                  int32_t *not_off, int32_t *nots2) {
    if (!shared_with || !ranks_out || !lin_sizes2 || !lin_level_off || !lin_launch_off || !lin_launch_rank || !lins35 ||
        !not_off || !nots2) {
        set_error("test_level_plan_full: null output");
        return -1;
    }
    if (ndead < 0 || (ndead > 0 && !dead_slots)) { set_error("test_level_plan_full: bad dead_slots"); return -1; }
    if (nterms < 0 || (nterms > 0 && !lin_terms2)) { set_error("test_level_plan_full: bad term table"); return -1; }
    const TestLinPlan lin{lin_terms2, nterms, ranks_out, lin_sizes2, lin_level_off, lin_launch_off, lin_launch_rank, lins35,
                          not_off, nots2};
    return test_level_plan(ops16, op_keys, count, nkeys, unit, balance, levels_out, sizes6, rot_off, ks_off, rot_koff, ks_koff,
                           rot_key, rots10, 10, kss4, true, reuse, shared_with, 16, dead_slots, ndead, &lin);
}

int tfhe_hip_test_br_plan(int32_t N, int32_t l, int32_t Bgbit, const int32_t *tunings4, int32_t cu_count, int32_t count,
                          int32_t flags, int32_t *out3) {
    if (!tunings4 || !out3 || cu_count < 1 || count < 1) { set_error("test_br_plan: bad arguments"); return -1; }
    LaunchTunings t;
    t.br_variant = tunings4[0]; t.br8_max_rotations = tunings4[1]; t.br_tail8 = tunings4[2]; t.br_digit_table = tunings4[3];
    bool form_ok[BR_FORM_COUNT][3];
    fill_form_ok(form_ok, N, l, Bgbit);                       // as upload_key fills a key image's
    const BrPlan plan = plan_br(form_ok, N, l, t, cu_count, count, (flags & 1) != 0, (flags & 2) != 0);
    out3[0] = plan.form; out3[1] = plan.tables; out3[2] = plan.tail;
    return 0;
}

int tfhe_hip_test_ks_plan_form(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings5,
                               int32_t cu_count, int32_t count, int64_t *out7) {
    if (!tunings5 || !out7 || cu_count < 1 || count < 1) { set_error("test_ks_plan: bad arguments"); return -1; }
    LaunchTunings t;
    t.ks_target_blocks = tunings5[0]; t.ks_max_splits = tunings5[1]; t.ks_split_ties = tunings5[2];
    t.ks_tile = tunings5[3]; t.ks_index = tunings5[4];
    Params p{};
    p.n = n;
    const KsShape shape{k * N, ks_t, ks_basebit, p.ct_stride()};
    const KsPlan plan = plan_ks(t, count, shape);             // what Engine::launch_ks runs
    const bool tiled = plan.form != KS_FORM_PERGATE;
    const int chunk = tiled ? KS_CHUNK : count;               // launch_ks's chunks: all of `chunk` gates but the last
    out7[0] = tiled ? 1 : 0;
    out7[1] = plan.tile;
    out7[2] = chunk;
    out7[3] = ks_splits(t, cu_count, std::min(chunk, count), shape);
    out7[4] = ks_splits(t, cu_count, count - (count - 1) / chunk * chunk, shape);
    out7[5] = (int64_t)ks_partial_bytes(t, cu_count, count, shape);
    out7[6] = plan.form;
    return 0;
}

// the first six words of the entry above: callers of this one provide room for six
int tfhe_hip_test_ks_plan(int32_t n, int32_t N, int32_t k, int32_t ks_t, int32_t ks_basebit, const int32_t *tunings5,
                          int32_t cu_count, int32_t count, int64_t *out6) {
    int64_t out7[7];
    if (!out6) { set_error("test_ks_plan: bad arguments"); return -1; }
    const int rc = tfhe_hip_test_ks_plan_form(n, N, k, ks_t, ks_basebit, tunings5, cu_count, count, out7);
    if (rc == 0) std::copy(out7, out7 + 6, out6);
    return rc;
}

int tfhe_hip_test_wg_times(const TFheGateBootstrappingCloudKeySet *bk, int32_t width, uint64_t *times4, double *launch_ms) {
    if (!bk || !bk->bk || !times4 || width <= 0) { set_error("wg_times: bad arguments"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    const double ms = Engine::get().run_wg_times(bk->bk->dev, width, reinterpret_cast<unsigned long long *>(times4));
    if (launch_ms) *launch_ms = ms;
    if (ms < 0) { set_error("wg_times: the launched kernel form wrote no stamps"); return -1; }
    return 0;
}

int tfhe_hip_kernel_negacyclic(const TFheGateBootstrappingCloudKeySet *bk, const int32_t *ip, const Torus32 *tp,
                               Torus32 *res, int32_t count) {
    if (!bk || !bk->bk) { set_error("negacyclic: null keyset"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    Engine::get().run_negacyclic(bk->bk->dev, ip, tp, res, count);
    return 0;
}
int tfhe_hip_kernel_bootstrap_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                   Torus32 *u_out, Torus32 *acc_out) {
    if (!bk || !bk->bk) { set_error("bootstrap_woks: null keyset"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    Engine::get().run_raw_rotations(bk->bk->dev, lin, count, nullptr, nullptr, 0, nullptr, nullptr, 0, 1, u_out, acc_out, "bootstrap_woks");
    return 0;
}
int tfhe_hip_kernel_lut_bootstrap_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                       const int32_t *lut_index, const Torus32 *polys, int32_t npolys, Torus32 *u_out,
                                       Torus32 *acc_out) {
    if (!bk || !bk->bk) { set_error("lut_bootstrap_woks: null keyset"); return -1; }
    if (!lut_index || !polys || npolys < 1) { set_error("lut_bootstrap_woks: null or empty LUT table"); return -1; }
    auto g = recorder_lock();
    return guarded_rc([&] {
        pool_of_key(bk);
        Engine::get().run_raw_rotations(bk->bk->dev, lin, count, lut_index, polys, npolys, nullptr, nullptr, 0, 1, u_out, acc_out, "lut_bootstrap_woks");
        return 0;
    });
}
int tfhe_hip_kernel_lut_bootstrap_multi_woks(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *lin, int32_t count,
                                             const int32_t *lut_index, const Torus32 *polys, int32_t npolys,
                                             const int32_t *spec_index, const int32_t *specs, int32_t nspecs, Torus32 *u_out,
                                             Torus32 *acc_out) {
    if (!bk || !bk->bk) { set_error("lut_bootstrap_multi_woks: null keyset"); return -1; }
    if (!lut_index || !polys || npolys < 1) { set_error("lut_bootstrap_multi_woks: null or empty LUT table"); return -1; }
    if (!spec_index || !specs || nspecs < 1) { set_error("lut_bootstrap_multi_woks: null or empty spec table"); return -1; }
    static_assert(XS_WORDS == TFHE_HIP_EXTRACT_SPEC_WORDS, "the spec records of the raw entry are ExtractSpec's words");
    auto g = recorder_lock();
    return guarded_rc([&] {
        pool_of_key(bk);
        Engine::get().run_raw_rotations(bk->bk->dev, lin, count, lut_index, polys, npolys, spec_index, reinterpret_cast<const ExtractSpec *>(specs),
                                        nspecs, XS_MAX_OUT, u_out, acc_out, "lut_bootstrap_multi_woks");
        return 0;
    });
}
int tfhe_hip_kernel_keyswitch(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *u, int32_t count, Torus32 *out) {
    if (!bk || !bk->bk) { set_error("keyswitch: null keyset"); return -1; }
    auto g = recorder_lock();
    pool_of_key(bk);
    Engine::get().run_keyswitch(bk->bk->dev, u, count, out);
    return 0;
}

}  // extern "C"

// The host side of the packing key switch is compiled as part of this object too (it uses the array headers above).
#include "pack_host.cpp"
// and that of the ring-encrypted inputs, behind it (it uses the negacyclic product defined there)
#include "unpack_host.cpp"
// and that of the private selection, behind both (the TGSW encryptor uses the same product)
#include "select_host.cpp"

// and that of the seed-compressed cloud keys
#include "compressed_host.cpp"
// and that of the seed-compressed packing keys and ring samples (it uses the packing key and the unpack defined above)
#include "seeded_host.cpp"
// and that of the seed-compressed LWE sample arrays
#include "seeded_lwe_host.cpp"

// The recorder is compiled as part of this object.  build.sh is one of the files kernels_sha16 hashes (kernel_id.py): a new
// host source named there would mark every committed counter summary stale although no kernel changed.
#include "recorder.cpp"
