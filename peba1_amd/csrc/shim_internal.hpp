// shim_internal.hpp -- what the host entry files share: shim.cpp (the public C ABI) and the files it includes into its
// object (pack_host.cpp, unpack_host.cpp, select_host.cpp, compressed_host.cpp, seeded_host.cpp, seeded_lwe_host.cpp,
// test_entries.cpp, recorder.cpp), and the host files that are objects of their own (public_host.cpp, seeded_select_host.cpp, inner_sum_host.cpp, ring_rotate_host.cpp).  The object stays one because build.sh is one of the files kernels_sha16 hashes
// (kernel_id.py); every one of those files includes this header and whatever else it uses, and parses on its own
// (tests/test_host_sources_cpu.py), so the order of the include lines at the end of shim.cpp means nothing.
// Each cross-file function is defined in the file named above its declaration.
#pragma once
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "engine.hpp"
#include "recorder.hpp"
#include "../../include/tfhe/tfhe.h"

// rows [n][t][k+1][N] under a ring key; the device image is made at the first pack (a key can be built, read and
// deleted on a machine without a GPU)
struct TfheHipPackingKey {
    uint32_t magic;
    tfhe_hip::Params p;
    int32_t t, basebit;
    std::vector<Torus32> rows;
    tfhe_hip::DeviceBuf<uint32_t> img;       // empty until the first pack
    // a device-expanded key (tfhe_hip_expand_packing_key, seeded_host.cpp) holds the mask seed and the bodies alone: rows
    // stays empty until tfhe_hip_packing_key_words asks for the words
    std::vector<uint32_t> mask_seed; // [10] or empty (a plain key)
    std::vector<Torus32> body;       // [n][t][N]
};

// the rows [nbits][(k+1) l][k+1][N] of a selector; the device image is made at the first select (a selector can be built
// and deleted on a machine without a GPU)
struct TfheHipSelector {
    uint32_t magic;
    tfhe_hip::Params p;
    int32_t nbits;
    std::vector<Torus32> words;
    RingImage *img;
    // a compressed selector (tfhe_hip_new_selector_compressed, seeded_select_host.cpp) holds the mask seed and the bodies
    // alone: words stays empty, and only the bodies reach the card
    std::vector<uint32_t> mask_seed; // [10] or empty (a plain selector)
    std::vector<Torus32> body;       // [nbits][(k+1) l][N]
    int64_t upload_bytes;            // what the image's upload copied to the card; 0 until it is made
};

namespace tfhe_hip {

// ---- io.cpp ----
bool io_forget_owned_cloud(const void *ks);     // keysets created by the file loaders
bool io_forget_owned_secret(const void *ks);
TFheGateBootstrappingCloudKeySet *io_adopt_cloud(TfheHipCloudKey *ck);   // a cloud keyset of its own around ck

#pragma GCC visibility push(hidden)   // library-internal: the exported surface is the C ABI

// ---- shim.cpp: the array headers ----
// Hidden header in front of every LweSample array handed to the caller.
struct alignas(16) ArrayHeader {
    uint32_t magic;
    int32_t count;
    int32_t n;
    int32_t unused;
    SlotPool *pool;     // set when the first element moves to the device
};
ArrayHeader *header_of(const LweSample *sample);   // refuses (ApiError) a null sample or one that is not ours

// bootsSymEncrypt and the default keygen draw from two ChaCha20 streams keyed by the OS (host_keys.hpp: one for the noise /
// the secrets, one for the public masks); after tfhe_hip_set_encrypt_seed both roles fall to ONE seeded xoshiro generator
// (secret; the specified draw order of the fixtures).  Used under the recorder lock.
struct EncryptRng { Rng secret = Rng::secure(), mask = Rng::secure(); bool seeded = false; };
EncryptRng &enc_rng();

// ---- the entry wrappers ----
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

// a fresh ChaCha20 key and nonce from the OS
inline void os_seed(uint32_t seed[10]) {
    if (!os_random(seed, 10 * sizeof(uint32_t))) fatal("the operating system offers no entropy (getrandom, /dev/urandom)");
}

// ---- argument checks ----
// The results of an unpack or of a seeded import: consecutive samples from `base`, or the samples `list` points to.
struct ResultsView {
    LweSample *base = nullptr;
    LweSample *const *list = nullptr;
    ResultsView(LweSample *b) : base(b) {}
    ResultsView(LweSample *const *l) : list(l) {}
    explicit operator bool() const { return base || list; }
    LweSample *at(int32_t j) const { return list ? list[j] : base + j; }
    // as check_runs takes `count` results: one run of that length, or count runs of one
    int32_t runs(int32_t count) const { return list ? count : 1; }
    int32_t run_length(int32_t count) const { return list ? 1 : count; }
};

// Argument checks the pack, unpack and seeded-import entries share; w: "entry name: ".
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
inline void check_runs(const std::string &w, const RunMessages &say, const ResultsView &result, int32_t count, const Params &p) {
    check_runs(w, say, [&](int32_t j) { return result.at(j); }, result.runs(count), result.run_length(count), p);
}

// an index list, or -- index null -- 0 .. count - 1, which `storage` then holds
inline const int32_t *index_or_iota(const int32_t *index, int32_t count, std::vector<int32_t> &storage) {
    if (index) return index;
    storage.resize((size_t)count);
    std::iota(storage.begin(), storage.end(), 0);
    return storage.data();
}
// The coefficient list of an unpack of nring ring samples of N: every index inside them, or -- index null -- 0 .. count - 1,
// which `iota` then holds.  at: the refusal of an index names its position and the range
inline const int32_t *ring_index_checked(const std::string &w, const int32_t *index, int32_t count, int32_t nring, int32_t N, bool at,
                                         std::vector<int32_t> &iota) {
    if (count < 1 || nring < 1) api_fail(w + "count and nring must be at least 1");
    const int64_t ncoef = (int64_t)nring * N;
    if (ncoef > INT32_MAX) api_fail(w + "nring * N must stay below 2^31");
    if (!index && count > ncoef) api_fail(w + "count runs past the last coefficient of the ring samples");
    for (int32_t j = 0; index && j < count; ++j)
        if (index[j] < 0 || index[j] >= ncoef)
            api_fail(at ? w + "index " + std::to_string(index[j]) + " at " + std::to_string(j) + " is outside 0.." + std::to_string(ncoef - 1)
                        : w + "index " + std::to_string(index[j]) + " is out of range");
    return index_or_iota(index, count, iota);
}

// ---- one slot transaction for the imports that make their samples on the device (unpack, seeded import) ----
// `count` fresh slots of `pool`; fill(slots) -- the engine call -- writes them; then the results are re-pointed to them
// and, in immediate mode, their mirrors refreshed.  When the pool or the device is full (ApiError) nothing was enqueued:
// what was taken is released and nothing has changed.  Under the recorder lock, the argument checks behind the caller.
template <typename Fill>
void import_into_fresh_slots(SlotPool *pool, const ResultsView &result, int32_t count, Fill &&fill) {
    std::vector<int32_t> slots;
    slots.reserve((size_t)count);
    try {
        for (int32_t j = 0; j < count; ++j) slots.push_back(alloc_slot(pool));
        fill(slots.data());
    } catch (const ApiError &) {
        for (int32_t s : slots) pool->release(s);
        throw;
    }
    for (int32_t j = 0; j < count; ++j) repoint(result.at(j), pool, slots[(size_t)j]);
    if (!deferred_mode())
        for (int32_t j = 0; j < count; ++j) sync_sample_locked(result.at(j));
}

// ---- pack_host.cpp ----
// body += mask * key in Z[X]/(X^N + 1), key binary; sign = -1 subtracts
void pack_add_mul_by_bits(uint32_t *body, const uint32_t *mask, const int32_t *bits, int N, uint32_t sign);
// 0, 0 = the set's own key-switch decomposition; null if the pair is refused (the error is set)
// with_rows false: the rows stay empty (a device-expanded key, seeded_host.cpp)
TfheHipPackingKey *new_packing_key_object(const char *who, const Params &p, int32_t pk_t, int32_t pk_basebit, bool with_rows = true);
bool pack_same_set(const Params &a, const Params &b);
const TfheHipPackingKey *pack_key_checked(const char *who, const TfheHipPackingKey *key);   // ApiError: null or deleted
// the key's image, made at first use (under the recorder lock, the cloud key's image in place)
const uint32_t *pack_image(const TfheHipPackingKey *ckey, const TFheGateBootstrappingCloudKeySet *bk);
// [n][t][2][N] from seed and bodies [n][t][N]: the mask polynomials are consecutive stretches of one sequential stream
void expand_packing_rows_host(const Params &p, int t, const uint32_t seed10[10], const Torus32 *body, std::vector<Torus32> &rows);

// ---- select_host.cpp ----
// An empty selector of nbits bits for an accepted parameter set; null, the error set under the prefix w, for what
// tfhe_hip_new_selector refuses: a null set, nbits outside 0..SELECT_MAX_BITS, a set no cloud key is accepted with, a
// gadget outside the CMUX kernel's two bounds.
TfheHipSelector *new_selector_object(const std::string &w, const TFheGateBootstrappingParameterSet *params, int32_t nbits);
bool selector_ok(const TfheHipSelector *sel);       // not null, not deleted
const TfheHipSelector *selector_checked(const std::string &w, const TfheHipSelector *sel);   // ApiError: null or deleted
// the selector's image, made at first use (under the recorder lock); null for a selector of no bits
const RingImage *select_image(const TfheHipSelector *sel);

// ---- unpack_host.cpp ----
// msg = the N coefficients that encode `count` bits (+-1/8, then zeros); false, the error set, unless count is in 1..N
bool ring_message_of_bits(const char *who, const int32_t *bits, int32_t count, int N, std::vector<Torus32> &msg);
// seeded: `ring` holds seed-compressed records (seeded_host.cpp)
int unpack_impl(const char *who, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring, int32_t nring,
                const int32_t *index, int32_t count, ResultsView result, bool device_src, bool seeded = false);
// the body of tfhe_hip_kernel_ring_extract and tfhe_hip_kernel_ring_extract_seeded
int ring_extract_impl(const char *who, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring, int32_t nring,
                      const int32_t *index, int32_t count, Torus32 *u_out, bool seeded);

#pragma GCC visibility pop
}  // namespace tfhe_hip
