// shim.cpp -- the public C ABI of libtfhe-hip: the tfhe boots* surface that
// /root/reference/src/Math.cpp and src/main.cpp bind plus the
// tfhe_hip_* extensions.  Host logic only: the array headers, keys, I/O glue, tunings and statistics; the
// boots* gate entries hand over to the recorder (recorder.hpp).  No gate arithmetic happens here.  The entries of the later
// features and of the tests are in the files included at the end; what they share with this one is in shim_internal.hpp.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "scheduler.hpp"
#include "shim_internal.hpp"

using namespace tfhe_hip;

namespace {

constexpr uint32_t ARRAY_MAGIC = 0x7F4E11A5u;

// Every sample's host mirror is preceded by a back-pointer to its array's header and a marker, so
// the pool a sample lives in can be found from any element pointer (&array[i]).  The marker is
// checked BEFORE the back-pointer is followed.  Why it matters: the reference's Function_g writes
// bitsize+1 results into a bitsize-sample array (Math.cpp:399-401).  That "sample" one
// past the end overlays the first mirror prefix of the block, so its `a` field reads as the
// back-pointer (the block's own start): the words in front of THAT are the allocator's chunk header
// -- readable, and not the marker -- and the call is refused instead of following garbage.
constexpr int MIRROR_PREFIX_WORDS = 4;   // one pointer + marker (8 bytes)
constexpr uint64_t MIRROR_MARKER = 0x7F4E5A3D1E5AA11Cull;

void record_gate2(int code, LweSample *result, const LweSample *ca, const LweSample *cb,
                  const TFheGateBootstrappingCloudKeySet *bk) {
    guarded([&] {
        auto g = recorder_lock();
        record_gate2_locked(code, result, ca, cb, bk);
    });
}

}  // namespace

ArrayHeader *tfhe_hip::header_of(const LweSample *sample) {
    uint64_t marker;
    ArrayHeader *h;
    if (!sample || !sample->a) api_fail("LweSample was not allocated by new_gate_bootstrapping_ciphertext_array");
    std::memcpy(&marker, sample->a - 2, sizeof marker);
    if (marker != MIRROR_MARKER) api_fail("LweSample was not allocated by new_gate_bootstrapping_ciphertext_array");
    std::memcpy(&h, sample->a - MIRROR_PREFIX_WORDS, sizeof h);
    if (!h || h->magic != ARRAY_MAGIC) api_fail("LweSample was not allocated by new_gate_bootstrapping_ciphertext_array");
    return h;
}

EncryptRng &tfhe_hip::enc_rng() { static EncryptRng e; return e; }

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

// Unlike the imports that make their samples on the device (import_into_fresh_slots), this one re-points each sample as
// it allocates: the old slot of sample i is free for sample i + 1, so a re-import into a live array needs no more of the
// pool than it holds.  The price, a known hole: a refusal in the middle of the loop (the pool cannot grow) leaves the
// earlier samples renamed to slots nothing was written to.
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
    if (name && std::strcmp(name, "ks_matrix") == 0) { Engine::get().tunings.ks_matrix = value != 0; return 0; }
    if (name && std::strcmp(name, "ks_matrix_min") == 0) {
        if (value < 1 || value > (1 << 30)) { set_error("ks_matrix_min must be in [1, 2^30]"); return -1; }
        Engine::get().tunings.ks_matrix_min = (int)value;
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
    Engine::get().ks_matrix_stats = TfheHipKsMatrixStats{};
    Engine::get().seeded_stats = TfheHipSeededStats{};
    Engine::get().seeded_lwe_stats = TfheHipSeededLweStats{};
}
void tfhe_hip_get_seeded_stats(TfheHipSeededStats *out) {
    auto g = recorder_lock();
    if (out) *out = Engine::get().seeded_stats;
}
void tfhe_hip_get_ks_matrix_stats(TfheHipKsMatrixStats *out) {
    auto g = recorder_lock();
    if (out) *out = Engine::get().ks_matrix_stats;
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

}  // extern "C"

// The host side of every later feature, the test entries and the recorder are compiled as part of this object: build.sh is
// one of the files kernels_sha16 hashes (kernel_id.py), and a new host source named there would mark every committed
// counter summary and cost table stale although no kernel changed.  Each file includes what it uses (shim_internal.hpp):
// the order of these lines means nothing.
#include "pack_host.cpp"
#include "unpack_host.cpp"
#include "select_host.cpp"
#include "compressed_host.cpp"
#include "seeded_host.cpp"
#include "seeded_lwe_host.cpp"
#include "test_entries.cpp"
#include "recorder.cpp"
