// engine.hpp -- device side of libtfhe-hip: the resident evaluation key, the
// ciphertext slot pool and batched level execution on one HIP stream.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <string>
#include <vector>

#include "device_buf.hpp"
#include "host_keys.hpp"
#include "host_stage.hpp"
#include "br_forms.hpp"
#include "launch_plan.hpp"
#include "kernels.hpp"
#include "pack.hpp"
#include "unpack.hpp"
#include "cmux.hpp"
#include "expand.hpp"
#include "ks_matrix.hpp"
#include "ring_public.hpp"
#include "ring_inner_sum.hpp"
#include "ring_rotate.hpp"
#include "../../include/tfhe_hip.h"

// Device image of one cloud key: NTT image of BK, compact KSK, twiddles.
struct DeviceKeyImage {
    tfhe_hip::DevParams dp;
    tfhe_hip::DevKey key;
    // form_ok[form][tables]: the kernel form's magnitude bounds hold for this key's (l, Bgbit) (br_forms.hpp)
    bool form_ok[tfhe_hip::BR_FORM_COUNT][3] = {};
    tfhe_hip::DeviceBuf<uint32_t> bk_img;
    tfhe_hip::DeviceBuf<int32_t> ksk;
    tfhe_hip::DeviceBuf<uint32_t> tw;
    // the byte-plane image of the KSK for the matrix key switch (ks_matrix.hip), made before the first flush with a launch
    // wide enough to use it (Engine::ensure_ks_planes); empty until then, and for good on a card without room for it
    mutable tfhe_hip::DeviceBuf<uint8_t> ks_planes;
};
// Device image of an object that belongs to a parameter set, not to a cloud key, and so carries the ring's twiddle tables
// itself: the NTT image of a selector's rows (Engine::upload_selector) or of a public gallery's polynomials (upload_public)
struct RingImage { tfhe_hip::DeviceBuf<uint32_t> img, tw; };

namespace tfhe_hip {

void set_error(const std::string &msg);
const std::string &last_error_ref();
[[noreturn]] void fatal(const std::string &msg);
void hip_check(hipError_t e, const char *what);
const char *unsupported_reason(const Params &p);   // why the kernels cannot run this parameter set exactly, or null

// A condition the caller can recover from (slot pool exhausted, a sample this library did not
// allocate, a sample used with a key of another LWE dimension, a malformed file): thrown inside
// the library, caught at every extern "C" entry, reported through tfhe_hip_last_error() with
// the call left without effect.  fatal() (abort, like upstream) is kept for HIP runtime
// failures and for "no GPU", after which nothing can work.
struct ApiError { std::string msg; };
// test hook: device allocations of the slot pool and the flush scratch beyond `bytes` in total fail like hipErrorOutOfMemory
// (recoverably: engine.cpp recoverable_alloc); 0 = no cap
void set_alloc_cap(long long bytes);
long long alloc_held();                         // test hook: the bytes those allocations hold now
[[noreturn]] void api_fail(const std::string &msg);

// Pool of device-resident ciphertext slots (ct_stride words each).  Slots are
// immutable once written (the recorder renames every destination), reference
// counted, and recycled through a free list.
// the most slots a pool may hold (TFHE_HIP_POOL_SLOTS is clamped to it)
constexpr size_t MAX_POOL_SLOTS = (size_t)1 << 29;
// the most samples one export or import may name (write_ / read_slots_packed refuse more; include/tfhe_hip.h states it)
constexpr int MAX_PACKED_SAMPLES = 1 << 16;

class SlotPool {
public:
    SlotPool(int ct_words, int ct_stride, size_t capacity);
    ~SlotPool();
    int32_t alloc();                 // refcount 1, level 0
    void retain(int32_t s) { ++ref_[s]; }
    int32_t refs(int32_t s) const { return ref_[s]; }
    void release(int32_t s);
    int32_t *data() { return data_; }
    int ct_stride() const { return stride_; }
    int ct_words() const { return words_; }
    size_t capacity() const { return max_cap_; }              // what the pool may grow to
    size_t allocated() const { return cap_; }                 // slots backed by device memory now
    size_t in_use() const { return cap_ - free_.size(); }
    std::vector<int32_t> level;      // level of the recorded operation that will write the slot (0: an input)
    std::vector<uint8_t> pending;    // 1 = written by a recorded operation that has not run yet
    int32_t const_slot[2] = {-1, -1};   // shared read-only trivial samples (0, -1/8) and (0, +1/8)
private:
    void grow(size_t new_cap);
    int words_, stride_;
    size_t cap_ = 0, max_cap_;
    int32_t *data_ = nullptr;
    std::vector<int32_t> ref_;
    std::vector<int32_t> free_;
};

struct LevelPlan {
    // descriptors of the whole flush, ordered by level
    std::vector<RotDesc> rots;
    std::vector<KsDesc> kss;
    std::vector<NotDesc> nots;
    int levels = 0;
    std::vector<int32_t> rot_off, ks_off;   // size levels + 1; gates of level L (1-based): index L - 1
    std::vector<int32_t> not_off;           // size levels + 2; NOTs riding on level L (0 = inputs): index L
    // linear combinations (tfhe_hip_linear; all empty without one), ordered by (level, rank): the launches of level L
    // (0 = inputs) are [lin_level_off[L], lin_level_off[L + 1]) (size levels + 2), launch j runs the descriptors
    // [lin_launch_off[j], lin_launch_off[j + 1]) and holds the ops of rank lin_launch_rank[j]; a level's launches go in
    // this order behind its NOTs.  op_rank: the rank of every op of the flush (0 for all but linear combinations)
    std::vector<LinDesc> lins;
    std::vector<int32_t> lin_level_off, lin_launch_off, lin_launch_rank, op_rank;
    int32_t max_rots = 0;                   // widest level, in rotations
    int32_t max_extracts = 0;               // the most extracted samples of a level (sizes the extract buffer): max_rots,
                                            // or more with multi-output rotations
    // several cloud keys of one parameter set (recorder "batch_keys"; nkeys > 1 only): the key index of every rotation,
    // and the descriptors of level L (1-based) under key k at [rot_koff / ks_koff][(L - 1) nkeys + k, ... + 1)
    int nkeys = 1;
    std::vector<int32_t> rot_key;
    std::vector<int32_t> rot_koff, ks_koff;
    std::vector<tfhe_hip::DevKey> dev_keys; // the key table execute() uploads (held until the upload has happened)
};

class Engine {
public:
    static Engine &get();
    void ensure_init();
    int device() const { return device_; }
    int cu_count() const { return cu_count_; }
    void set_device(int d);
    hipStream_t stream() const { return stream_; }

    DeviceKeyImage *upload_key(const TfheHipCloudKey &ck);
    // The image of a device-expanded keyset (ck.mask_seed set; expand.hpp): the bodies are uploaded, the two expand kernels
    // write the raw BK staging buffer and the compact KSK from the seed, launch_bk_transform follows.  Every buffer is
    // allocated before anything is enqueued: device memory exhausted = ApiError with nothing held, as upload_key.
    DeviceKeyImage *upload_compressed_key(const TfheHipCloudKey &ck);
    double last_expand_ms = -1.0;       // the two expand kernels of the last such upload between stream events (kernel timing on)
    void free_key(DeviceKeyImage *img);
    // test paths: stream words through the kernels' block function; an uploaded key's BK image (which = 0) or compact KSK,
    // padding and zero row included (which = 1), copied back -- returns the word count, copies only if it fits `capacity`
    void run_expand_masks(const uint32_t seed10[10], int64_t first_word, int count, uint32_t *out);
    size_t read_key_image(const DeviceKeyImage *img, int which, Torus32 *out, size_t capacity);
    SlotPool *pool_for(const Params &p);
    SlotPool *find_pool(const Params &p) const;   // the pool of this ciphertext shape if one exists; never initialises the device

    void write_slot(SlotPool *pool, int32_t slot, const Torus32 *a, Torus32 b);       // host -> device
    void read_slot(SlotPool *pool, int32_t slot, Torus32 *a, Torus32 *b);             // device -> host
    // wait = false (device words only): the transfer is enqueued on the engine's stream and the call returns -- whatever
    // is enqueued on that stream afterwards (a collective, the next flush) is ordered behind it without a host wait
    void write_slots_packed(SlotPool *pool, const int32_t *slots, int count, const Torus32 *words, bool words_on_device, bool wait = true);
    void read_slots_packed(SlotPool *pool, const int32_t *slots, int count, Torus32 *words, bool words_on_device, bool wait = true);

    // run a levelised plan under the flush's keys (plan.nkeys of them, all of one parameter set and resident; the plan's
    // key indices refer to this list).  wait = true: synchronises the stream before returning; false: returns with the
    // launches enqueued ("in flight") -- see engine.cpp
    void execute(const std::vector<const DeviceKeyImage *> &keys, SlotPool *pool, LevelPlan &&plan, bool wait = true);
    int last_flush_keys = 0;            // distinct cloud keys of the last flush executed (tfhe_hip_last_flush_keys)
    void wait_flight();                 // completes an asynchronous execute(): waits, then reads the timing events
    // host waits (engine.cpp "host waits"): bounded by sync_deadline_ms when that is set
    void sync_stream(const char *what); // everything enqueued on the engine's stream has completed
    void sync_io() { stage_.wait(); }   // the stream-ordered transfers nobody waited for have completed
    void wait_all() { wait_flight(); sync_io(); }
    // a caller's event, bounded like the waits above (deadline and label passed in: read by the caller under the recorder lock)
    void wait_event(hipEvent_t ev, const char *what, long long deadline_ms, const std::string &label);
    bool pci_bus_id(char *out, int len);                // "0000:c1:00.0" of the engine's device
    // > 0: no host wait on the engine's stream lasts longer -- on expiry the process prints what it waited for and ends
    // with TFHE_HIP_EXIT_DEADLINE (tuning "sync_deadline_ms", env TFHE_HIP_SYNC_DEADLINE_MS); 0 = wait for ever
    long long sync_deadline_ms = 0;
    std::string diag_label;             // who waits, for the deadline message (tfhe_hip_set_diag_label: "rank 3 of 8")
    bool in_flight() const { return in_flight_; }
    // The table of caller-supplied test polynomials (tfhe_hip_new_lut): LUT_STRIDE words per entry in one device array
    // that doubles on demand; RotDesc::lut indexes it.  lut_add copies n_ring words in and returns the entry (an entry
    // freed earlier, or a new one); device memory exhausted while the table grows: ApiError, nothing changed.  lut_free
    // gives the entry back -- the caller has run every recorded op that names it (recorder.cpp forget_lut_locked).
    int32_t lut_add(const Torus32 *words, int n_ring);
    void lut_free(int32_t index);
    // The table of extract specs (tfhe_hip_new_lut_multi), the same mechanism (engine.cpp DeviceTable) over ExtractSpec
    // entries; RotDesc::spec indexes it.  The spec has passed extract_spec_error for its ring.
    int32_t spec_add(const ExtractSpec &xs);
    void spec_free(int32_t index);
    // raw test paths.  The one blind-rotate path of the three *bootstrap*_woks entries: `count` combinations of lin through
    // one planned launch from call-owned tables.  lut_index / polys / npolys (all or none): combination c starts from test
    // polynomial lut_index[c] of polys[npolys][N] (uploaded for this call only; an index below 0: the constant test
    // vector).  spec_index / specs / nspecs (all or none): it leaves through specs[spec_index[c]] (uploaded for this call
    // only, every output wanted; an index below 0, or no specs: the extract at index 0).  The device writes the outputs of
    // all combinations back to back (u_index = outputs before it); u_out[count][out_rows][kN+1] receives output m of
    // combination c at [c][m], the rest is left as it was.  name: the entry, for error messages
    void run_raw_rotations(const DeviceKeyImage *key, const Torus32 *lin, int count, const int32_t *lut_index,
                           const Torus32 *polys, int npolys, const int32_t *spec_index, const ExtractSpec *specs, int nspecs,
                           int out_rows, Torus32 *u_out, Torus32 *acc_out, const char *name);
    void run_keyswitch(const DeviceKeyImage *key, const Torus32 *u, int count, Torus32 *out);
    // raw test path of the matrix key switch alone (ks_matrix.hip), whatever the width; ApiError where the key's shape has no
    // matrix form or the card no room for its image
    void run_keyswitch_matrix(const DeviceKeyImage *key, const Torus32 *u, int count, Torus32 *out);
    // the key's byte-plane image, made on first need; false (and nothing held, nothing reported) if the shape has no matrix
    // form or the device has no room: the key then goes on with the other forms
    bool ensure_ks_planes(const DeviceKeyImage *key);
    void run_negacyclic(const DeviceKeyImage *key, const int32_t *ip, const Torus32 *tp, Torus32 *res, int count);
    // Packing key switch (pack.hpp).  upload_pack_image: the NTT image of a packing key's raw rows [n][t][2][N] under the
    // twiddles of `key` (a cloud key of the same ring); device memory exhausted: ApiError, nothing held.
    DeviceBuf<uint32_t> upload_pack_image(const DeviceKeyImage *key, const Torus32 *rows, int t);
    // The same image for a key that holds a mask seed and bodies [n][t][N] alone (tfhe_hip_expand_packing_key): the bodies go
    // up through the pinned staging area (half the bytes of the raw rows), launch_expand_bk (rows = n t, k = 1) writes the raw
    // staging buffer -- masks from the stream, bodies from the upload -- and launch_bk_transform follows.  All three buffers
    // are allocated before anything is enqueued: device memory exhausted = ApiError with nothing held.
    DeviceBuf<uint32_t> expand_pack_image(const DeviceKeyImage *key, const uint32_t seed10[10], const Torus32 *body, int t);
    void free_pack_image(DeviceBuf<uint32_t> &img);
    // test path: a packing key's image copied back -- returns the word count, copies only if it fits `capacity`
    size_t read_pack_image(const DeviceBuf<uint32_t> &img, Torus32 *out, size_t capacity);
    // One pack of `count` samples, enqueued on the engine's stream behind whatever is there.  slots (the slot form): sample
    // j is pool slot slots[j]; raw_words (the test form, slots null): sample j is raw_words[j][n + 1], uploaded for this
    // call.  idx_per_wg: mask indices per workgroup, 0 = the engine's choice.  out: 2N words, host or device; a host
    // destination, or wait, makes the call return with the words in place.
    void run_pack(const DeviceKeyImage *key, const uint32_t *img, int t, int basebit, SlotPool *pool, const int32_t *slots,
                  const Torus32 *raw_words, int count, int idx_per_wg, Torus32 *out, bool out_on_device, bool wait);

    // Ring-encrypted inputs (unpack.hpp): coefficient index[j] = r N + e of the nring ring samples ring_words (host, or
    // device memory the caller keeps until the stream has passed) becomes Extract_e, in chunks of at most UNPACK_CHUNK.
    // The slot form (u_out null): the key switch of row j goes straight into pool slot slots[j]; wait = false returns with
    // the work enqueued on the engine's stream.  The raw test form (u_out [count][kN+1]): the extract kernel's rows alone,
    // no key switch.  The caller has checked every index and waited for the flight.  Every buffer is sized before
    // anything is enqueued: an ApiError (device memory exhausted) leaves nothing written.
    // seeded: ring_words holds seed-compressed records of RING_SEED_WORDS + N words, opened by the seeded extract kernel.
    void run_unpack(const DeviceKeyImage *key, const Torus32 *ring_words, int nring, bool ring_on_device, const int32_t *index,
                    int count, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait, bool seeded = false);

    // test path: the padded rows the last extract launch wrote, [rows][u_stride] as the kernel stored them -- returns the
    // word count, copies only if it fits `capacity`
    size_t read_extract_rows(Torus32 *out, size_t capacity);

    // Seed-compressed LWE sample arrays (expand.hpp LweExpandArgs): row j becomes sample index[j] of the record whose
    // LWE_SEED_WORDS + record_count words lie at `record` (host, or device memory the caller keeps until the stream has
    // passed), in chunks of at most LWE_EXPAND_CHUNK, written by lwe_expand_kernel alone.  From a host record the seed, the
    // bodies the index names and the lists go up through the pinned staging area: count words, not count (n + 1).
    // The slot form (rows_out null): row j goes straight into pool slot slots[j]; wait = false returns with the work
    // enqueued on the engine's stream.  The raw test form (pool null, rows_out [count][n + 1]): into scratch rows, read back.
    // The caller has checked every index.  Every buffer is sized before anything is enqueued: an ApiError (device memory
    // exhausted) leaves nothing written.
    void run_lwe_expand(int n, int stride, const Torus32 *record, bool record_on_device, const int32_t *index, int count,
                        SlotPool *pool, const int32_t *slots, Torus32 *rows_out, bool wait);
    // test path: the scratch rows of the last raw expand launch, [rows][stride] as the kernel stored them -- returns the
    // word count, copies only if it fits `capacity`
    size_t read_expand_slots(Torus32 *out, size_t capacity);

    TfheHipStats stats{};
    TfheHipExpandStats expand_stats{};  // the device expansions of seed-compressed cloud keys (tfhe_hip_get_expand_stats)
    TfheHipKsMatrixStats ks_matrix_stats{};  // launches of the matrix key switch (tfhe_hip_get_ks_matrix_stats)
    TfheHipSeededStats seeded_stats{};  // device-expanded packing keys and seeded unpacks (tfhe_hip_get_seeded_stats)
    bool kernel_timing = false;
    // the launch rules' tunings (launch_plan.hpp; written by ensure_init()'s environment reads and tfhe_hip_set_tuning)
    LaunchTunings tunings;
    // the launch plan (launch_plan.hpp plan_ks_launch) of the key switches of `count` gates under this key's parameter set
    // on this card; has_image: the key holds its byte-plane image and the caller is a flush
    KsLaunchPlan plan_ks_launch(const DeviceKeyImage *key, int count, bool has_image) const;
    // runs a plan of plan_ks_launch on its plan.count descriptors: one kernel launch per part; decides nothing.  The caller
    // sized S_KS_PARTIAL from plan.partial_bytes before it enqueued anything (checked); stream == nullptr: the engine's
    void launch_ks(const DeviceKeyImage *key, const KsLaunchPlan &plan, const int32_t *u_buf, const KsDesc *descs, int32_t *pool,
                   hipStream_t stream = nullptr);
    // the launch plan (launch_plan.hpp plan_br) of `count` rotations under this key's parameter set on this card;
    // acc_dump: the raw accumulators are read back
    BrPlan plan_br_launch(const DeviceKeyImage *key, int count, bool acc_dump) const;
    // What one blind-rotate launch works on.  mk_keys / mk_rot_keys (device key table and per-rotation key indices of a
    // multi-key level): the 4- and 8-wave forms run each rotation under its own key; only for those forms, and `key` is
    // entry 0 of the table.  mid: where the event between the two launches of a plan with a tail goes (kernel timing of a
    // flush).  luts / specs: the tables the descriptors' lut and spec indices refer to; null = the engine's own
    struct BrLaunch {
        const int32_t *pool;
        const RotDesc *rots;
        int count;
        int32_t *u_buf;
        int32_t *acc_dbg = nullptr;
        hipStream_t stream = nullptr;            // null: the engine's stream
        const DevKey *mk_keys = nullptr;
        const int32_t *mk_rot_keys = nullptr;
        hipEvent_t *mid = nullptr;
        const int32_t *luts = nullptr;
        const ExtractSpec *specs = nullptr;
    };
    // runs a plan of plan_br_launch on these descriptors: one kernel launch, two with a tail; decides nothing
    void launch_br(const DeviceKeyImage *key, const BrPlan &plan, const BrLaunch &a);
    // diagnostic (tools/wg_times.py): ONE 4-wave blind-rotate launch of `width` random gates whose workgroups stamp s_memtime
    // and s_memrealtime at start and end into wg_times[4 * width]; returns that launch's event time in ms (< 0: no stamps)
    double run_wg_times(const DeviceKeyImage *key, int width, unsigned long long *wg_times);

private:
    Engine() = default;
    // The grow-only device scratch buffers, by name.  "flush": sized by prepare_flush() and owned by the flush in flight
    // until wait_flight().  "raw": sized and used by a raw test path, which waits for the flight first and for its own
    // work before it returns.  "io": sized by write_/read_slots_packed, used on the stream behind any flight.
    enum Scratch : size_t {
        S_ROTS,           // flush, raw rotations: the rotation descriptors
        S_KS,             // flush, run_keyswitch: the key-switch descriptors
        S_NOTS,           // flush: the descriptors of the NOTs
        S_LINS,           // flush: the descriptors of the linear combinations
        S_SLOTS,          // io: the slot list of a packed transfer
        S_WORDS,          // io: the packed words of a host transfer
        S_EXTRACT,        // flush, raw rotations, run_keyswitch: the extracted samples
        S_RAW_POOL,       // raw rotations: the padded inputs; run_keyswitch: the padded results
        S_RAW_ACC,        // raw rotations: the accumulators read back
        S_NEGA_TP = S_RAW_POOL, S_NEGA_IP = S_RAW_ACC,     // run_negacyclic's two operands share those buffers
        S_NEGA_IMG,       // raw, run_negacyclic: the transform of tp
        S_NEGA_RES,       // raw, run_negacyclic: the products
        S_KS_PARTIAL,     // flush, run_keyswitch, run_unpack: partial sums of split key switches, sized from the plans launch_ks runs
        S_KEYS,           // flush of several keys: the key table
        S_ROT_KEYS,       // flush of several keys: the key index of every rotation
        S_RAW_LUTS,       // raw rotations: the call's own test polynomials
        S_RAW_SPECS,      // raw rotations: the call's own extract specs
        S_PROBE_POOL, S_PROBE_ROTS, S_PROBE_TIMES, S_PROBE_EXTRACT,     // run_wg_times only (it waits for the flight first)
        S_PACK_SLOTS,     // run_pack: the slot list
        S_PACK_RAW,       // run_pack, raw form: the caller's sample words
        S_PACK_PARTIAL,   // run_pack: the partial sums of the workgroups
        S_PACK_OUT,       // run_pack: the result on its way to a host destination
        S_UNPACK_RING,    // run_unpack: the ring words on their way from a host source
        S_UNPACK_INDEX,   // run_unpack: the index list
        S_UNPACK_KS,      // run_unpack, run_inner: the key-switch descriptors (row j -> slot j)
        S_UNPACK_EXTRACT, // run_unpack, run_inner: the extracted samples of one chunk
        S_EXPAND_WORDS,   // raw, run_expand_masks: the stream words
        S_LWE_RECORD,     // run_lwe_expand: the seed and the gathered bodies of a host record
        S_LWE_INDEX,      // run_lwe_expand: the index list
        S_LWE_SLOTS,      // run_lwe_expand: the slot list
        S_LWE_ROWS,       // raw, run_lwe_expand: the rows of one chunk in place of pool slots
        S_SELECT_RING,    // run_select, run_inner[_sum], run_inner_sum_mul: the ring words on their way from a host source; run_cmux: the d0 operands
        S_SELECT_A,       // run_select / run_lookup: the launches 0, 2, ... (ping), tree levels then rotations; run_cmux: the results; run_inner_sum_mul: the sums on their way to a host destination
        S_SELECT_B,       // run_select / run_lookup: the launches 1, 3, ... (pong)
        S_CMUX_D1,        // raw, run_cmux: the d1 operands
        S_PUBLIC_RING,    // run_public[_sum]_mul, run_public[_sum]_inner: the ring words on their way from a host source
        S_PUBLIC_OUT,     // run_public[_sum]_mul: the products on their way to a host destination
        S_ROTATE_RING,    // run_ring_rotate[_rows]: the ring words on their way from a host source
        S_ROTATE_INDEX,   // run_ring_rotate[_rows]: the ring index list
        S_ROTATE_SLOTS,   // run_ring_rotate[_rows]: the slot list of the LWE samples
        S_ROTATE_LWE,     // raw, run_ring_rotate[_rows]: the caller's LWE words in place of pool slots
        S_ROTATE_OUT,     // run_ring_rotate: the accumulators on their way to a host destination
    };
    void *scratch(Scratch idx, size_t bytes);
    // the same by element count (and `margin` bytes), and `count` elements between host and device on the engine's stream
    template <class T> T *scratch_as(Scratch idx, size_t count, size_t margin = 0) { return static_cast<T *>(scratch(idx, count * sizeof(T) + margin)); }
    template <class T> void h2d(T *dst, const T *src, size_t count, const char *what) {
        hip_check(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, stream_), what);
    }
    template <class T> void d2h(T *dst, const T *src, size_t count, const char *what) {
        hip_check(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, stream_), what);
    }
    // a host list the caller may release as soon as the call returns: up through the pinned staging area
    template <class T> void h2d_staged(T *dst, const T *src, size_t count, const char *what) {
        T *h = static_cast<T *>(stage_.reserve(count * sizeof(T)));
        std::copy(src, src + count, h);
        h2d(dst, h, count, what);
    }
    // size a buffer and fill it in one step -- never in a flush, a pack or an unpack: they size everything before they enqueue
    template <class T> T *scratch_upload(Scratch idx, const T *src, size_t count, const char *what) {
        T *d = scratch_as<T>(idx, count);
        h2d(d, src, count, what);
        return d;
    }
    // execute() in three steps (engine.cpp): everything that can throw, then the uploads, then one call per level
    struct FlushBuffers { RotDesc *rots; KsDesc *ks; NotDesc *nots; int32_t *u_buf; DevKey *keys; int32_t *rot_keys; LinDesc *lins; };
    FlushBuffers prepare_flush(const std::vector<const DeviceKeyImage *> &keys, LevelPlan &plan);
    void upload_flush(const FlushBuffers &fb, LevelPlan &&plan);
    void run_level(const std::vector<const DeviceKeyImage *> &keys, SlotPool *pool, const FlushBuffers &fb, int L, hipEvent_t &shared_end);
    // em / tail: a level whose last round went to the 8-wave form as a second launch (BrPlan::tail) -- the event between
    // the two launches and the rotations of the second, so that each kernel's time and count stay its own
    struct Timed { hipEvent_t e0, e1, e2; bool wide8; int nrot; hipEvent_t em = nullptr; int tail = 0; };
    // the one tail of the stream-ordered entries: the stream is waited for, or the staging area's event is left behind them
    void finish(bool host_wait, const char *what) { host_wait ? sync_stream(what) : stage_.uploaded(); }
    std::vector<Timed> flight_timed_;
    hipEvent_t flight_base_ = nullptr;
    LevelPlan flight_plan_;
    int flight_levels_ = 0;
    bool in_flight_ = false;
    std::chrono::steady_clock::time_point flight_t0_;
    size_t last_extract_words_ = 0;                     // rows * u_stride of the last extract launch (read_extract_rows)
    HostStage stage_{*this};                            // the host lists of calls that return without a wait (host_stage.hpp)
    int device_ = 0;
    int cu_count_ = 256;
    std::atomic<bool> inited_{false};
    hipStream_t stream_ = nullptr;
    unsigned long long *clock_acc_ = nullptr;           // kernel timing: shader-cycle / reference-tick sums (kernels.hpp)
    unsigned long long *wg_times_dbg_ = nullptr;        // set by the workgroup-time probe only
    size_t timing_used_ = 0;
    hipEvent_t next_timing_event();
    std::vector<hipEvent_t> timing_events_;             // kernel_timing: up to 3 per level + 1 base
    std::vector<int32_t> spec_nout_;                    // outputs of every entry (execute() checks the extract buffer with it)
    std::vector<SlotPool *> pools_;
    std::vector<void *> scratch_ptr_;
    std::vector<size_t> scratch_size_;
    // behind everything else, so that the members the flush path reads keep their places
    size_t last_expand_words_ = 0;                      // rows * stride of the last raw LWE expand launch (read_expand_slots)
    void run_keyswitch_rows(const DeviceKeyImage *key, const KsLaunchPlan &plan, const Torus32 *u, Torus32 *out, const char *name);
public:
    TfheHipSeededLweStats seeded_lwe_stats{};           // seeded imports and their expand launches (tfhe_hip_get_seeded_lwe_stats)

    // Private selection (cmux.hpp).  The device side of a selector: the NTT image of its rows [nbits][(k+1) l][2][N] (the
    // bootstrapping-key image with n = nbits) and the ring's twiddle tables -- a selector belongs to a parameter set, not
    // to a cloud key, so it carries its own.  Both buffers are allocated before anything is enqueued: device memory
    // exhausted = ApiError with nothing held.  free_selector waits for the stream first (a select in flight reads both).
    RingImage *upload_selector(const Params &p, const Torus32 *words, int nbits);
    // The same image from a seed-compressed selector (include/tfhe_hip.h "seed-compressed selectors"): bodies
    // [nbits][(k+1) l][N] go up through the pinned staging area, launch_expand_bk writes the masks of the staging rows from
    // the stream of seed10 (rows = nbits (k+1) l, from 2 l for one bit), the transform is upload_selector's.
    RingImage *upload_selector_seeded(const Params &p, const uint32_t seed10[10], const Torus32 *bodies, int nbits);
    void free_selector(RingImage *sel);
    // The CMUX tree over the M ring samples `ring` (host, or device memory the caller keeps until the stream has passed)
    // under the nbits selector bits of `sel` (null when nbits = 0: a copy), enqueued on the engine's stream behind
    // whatever is there: one launch per level, level j from entries of level j - 1 in one of two ping-pong buffers into
    // the other, the last one straight into a device destination.  Names no pool slot and waits for no flight.  Every
    // buffer is sized before anything is enqueued: an ApiError (device memory exhausted) leaves nothing written.  A host
    // source or destination makes the call return with the words in place; the device form returns with the work enqueued.
    void run_select(const RingImage *sel, const Params &p, int nbits, const Torus32 *ring, int M, bool ring_on_device,
                    Torus32 *out, bool out_on_device) {
        run_lookup(sel, p, nbits, ring, M, p.N, ring_on_device, out, out_on_device);
    }
    // The packed lookup (include/tfhe_hip.h): `ring` holds R = ceil(M / S) samples of S = N / width entries each.  The tree
    // above over the R samples under bits s .. nbits - 1 (s = log2 S), then one rotation launch per bit t < s, rot =
    // width 2^t, in the same two ping-pong buffers (each at least one sample), the last launch of all straight into a
    // device destination.  width = N is run_select: no rotation, every launch and every buffer as before.  The caller has
    // checked width, nbits >= s and M; everything else as for run_select.
    void run_lookup(const RingImage *sel, const Params &p, int nbits, const Torus32 *ring, int M, int width, bool ring_on_device,
                    Torus32 *out, bool out_on_device);
    // raw test path: `count` independent CMUXes under bit `bit` in ONE launch, host words in and out; rot != 0: `count`
    // rotation steps ROT(G_bit, rot, d0[c]) instead (d1 is not looked at)
    void run_cmux(const RingImage *sel, const Params &p, int bit, const Torus32 *d1, const Torus32 *d0, int count, Torus32 *out,
                  int rot = 0);
    // Encrypted inner products (include/tfhe_hip.h; cmux.hpp InnerArgs): `ring` holds R samples (host, or device memory the
    // caller keeps until the stream has passed) of S = N / width entries each, M of them real, (R - 1) S < M <= R S.  Entry
    // i becomes the row Extract_((i mod S) width)(G_bit (.) c_(i / S)) -- product and extraction in ONE launch per chunk of
    // at most UNPACK_CHUNK rows -- and then goes the way of run_unpack's rows, through the same code: the slot form (u_out
    // and prod_out null) key-switches row i into pool slot slots[i] under `key`; the raw form u_out [M][kN+1] returns the
    // rows alone (key may be null); the raw form prod_out [R][(k+1) N] the full products of one launch and no rows.
    // The caller has checked every argument and, for the slot form, waited for the flight.  Every buffer is sized before
    // anything is enqueued: an ApiError (device memory exhausted) leaves nothing written.
    void run_inner(const RingImage *sel, const Params &p, int bit, const DeviceKeyImage *key, const Torus32 *ring, int R,
                   bool ring_on_device, int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, Torus32 *prod_out,
                   bool wait);
    // Sums of TGSW products over `terms` ring samples (ring_inner_sum.hpp InnerSumArgs; include/tfhe_hip.h "TGSW products
    // over several ring samples"): `ring` holds G groups of `terms` samples, group g under the selector samples bit ..
    // bit + terms - 1.  run_inner_sum_mul: out[g] = sum_t G_(bit + t) (.) c_(g terms + t) for g < G in ONE launch, enqueued
    // behind whatever is on the stream; names no pool slot; a host source or destination makes the call return with the
    // words in place.  run_inner_sum: run_inner over groups -- entry i < M is the row Extract_((i mod S) width)(sum of group
    // i / S), (G - 1) S < M <= G S, a further row maker for run_rows: the same chunks, the same key-switch plans, the slot
    // form and the raw form u_out.  The caller has checked every argument (terms against inner_sum_max_terms among them).
    void run_inner_sum_mul(const RingImage *sel, const Params &p, int bit, int terms, const Torus32 *ring, int G, bool on_device,
                           Torus32 *out);
    void run_inner_sum(const RingImage *sel, const Params &p, int bit, int terms, const DeviceKeyImage *key, const Torus32 *ring, int G,
                       bool ring_on_device, int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait);
    // the launches of the last run_select / run_lookup between two stream events (kernel timing on; waits for the second), else -1;
    // after a run_inner: from its first product launch to its last (ONE launch up to UNPACK_CHUNK rows)
    double last_select_ms();

    // Ring sample times public polynomials (ring_public.hpp).  The device side of a public gallery: the canonical NTT
    // residues of its R polynomials under both primes, [R][2][N] (8 KB each), made by ONE launch of public_image_kernel at
    // upload, and the ring's twiddle tables -- a gallery belongs to a parameter set, not to a cloud key, so it carries its
    // own.  Every buffer is allocated before anything is enqueued: device memory exhausted = ApiError with nothing held.
    // free_public waits for the stream first (a product in flight reads both).
    RingImage *upload_public(int N, const int32_t *polys, int R);
    void free_public(RingImage *g);
    // The products q_(first + g * img_step) * c_(g * (broadcast ? 0 : 1)), g < total, of ring samples `ring` (host, or
    // device memory the caller keeps until the stream has passed), enqueued on the engine's stream behind whatever is
    // there in ONE launch.  nsamples: the samples `ring` holds (1: one sample under every polynomial).  Names no pool slot
    // and waits for no flight.  A host source or destination makes the call return with the words in place.
    void run_public_mul(const RingImage *g, int N, int first, int img_step, const Torus32 *ring, int nsamples, int total,
                        bool on_device, Torus32 *out);
    // The inner products of ONE probe sample with the gallery's polynomials 0 .. R - 1 (include/tfhe_hip.h): entry i < M is
    // the row Extract_((i mod S) width)(q_(i / S) * probe), product and extraction in ONE launch per chunk of at most
    // UNPACK_CHUNK rows, the rows then going the way of run_unpack's and run_inner's through the same code: the slot form
    // (u_out null) key-switches row i into pool slot slots[i] under `key`; the raw form u_out [M][kN+1] returns the rows
    // alone (key may be null).  The caller has checked every argument and, for the slot form, waited for the flight.
    void run_public_inner(const RingImage *g, const Params &p, const DeviceKeyImage *key, const Torus32 *probe, bool probe_on_device,
                          int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait);
    // Sums of products over `terms` ring samples (ring_public.hpp PublicSumArgs; include/tfhe_hip.h "public products over
    // several ring samples"): out[g] = sum_t q_(first + g terms + t) * c_t for g < ngroups in ONE launch, `ring` the
    // [terms][(k+1) N] words of the samples.  Everything else as run_public_mul.  The caller has checked the groups'
    // CRT bound.
    void run_public_sum_mul(const RingImage *g, int N, int first, int terms, int ngroups, const Torus32 *ring, bool on_device,
                            Torus32 *out);
    // run_public_inner over groups: entry i < M is the row Extract_((i mod S) width)(sum_t q_((i / S) terms + t) * probe_t),
    // a further row maker for run_rows -- the same chunks, the same key-switch plans.
    void run_public_sum_inner(const RingImage *g, const Params &p, const DeviceKeyImage *key, int terms, const Torus32 *probe,
                              bool probe_on_device, int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait);
    // Ring LUT bootstrap (ring_rotate.hpp; include/tfhe_hip.h "ring LUT bootstrap"): rotation j < count blind-rotates ring
    // sample ring_index[j] (a host list the caller has checked against nring; null: sample j) of `ring` (nring samples: host,
    // or device memory the caller keeps until the stream has passed) by an LWE sample under `key`, whose bootstrapping image
    // is read as it rests.  The LWE samples: pool slots in_slots[j] (a host list), or -- pool null -- the caller's host words
    // lwe_words [count][n + 1].  run_ring_rotate: ONE launch, ACC_n of every rotation to `out` (host or device); names no
    // pool slot of its own.  run_ring_rotate_rows: a further row maker for run_rows -- the row Extract_0(ACC_n) of every
    // rotation, one launch per chunk of at most UNPACK_CHUNK rows, the same chunks and key-switch plans as run_unpack: the
    // slot form (u_out null) key-switches row j into pool slot out_slots[j]; the raw form u_out [count][kN+1] returns the
    // rows alone.  The caller has checked every argument and, for the slot form, waited for the flight.  Every buffer is
    // sized before anything is enqueued: an ApiError (device memory exhausted) leaves nothing written.
    void run_ring_rotate(const DeviceKeyImage *key, const Torus32 *ring, int nring, bool ring_on_device, const int32_t *ring_index,
                         SlotPool *pool, const int32_t *in_slots, const Torus32 *lwe_words, int count, Torus32 *out, bool out_on_device);
    void run_ring_rotate_rows(const DeviceKeyImage *key, const Torus32 *ring, int nring, bool ring_on_device, const int32_t *ring_index,
                              SlotPool *pool, const int32_t *in_slots, const Torus32 *lwe_words, int count, const int32_t *out_slots,
                              Torus32 *u_out, bool wait);
    // the rotation launches of the last of those two calls between two stream events (kernel timing on; waits for the
    // second), else -1
    double last_ring_rotate_ms();
private:
    // The one upload path of the transformed images (engine.cpp upload_image).  ImageRows: what an image is made from --
    // `rows` rows of `polys` polynomials, raw at `host`, or with seed10 their bodies alone at `host` (staged: through the
    // pinned staging area, else a blocking copy).  ImageTexts: what the path's allocations are called in an out-of-memory
    // message, and its steps in a fatal one (refused: the whole text when launch_expand_bk takes no such arguments).  ImageStep:
    // the points at which a cloud key adds buffers and launches of its own -- the image allocated; the staging allocated too
    // (nothing enqueued yet); seeded only, the bodies up and launch_expand_bk next; the staging rows filled, the transform next
    struct ImageTexts { const char *img, *raw, *body, *upload, *expand, *refused, *transform, *sync; };
    struct ImageRows { int rows, polys; const Torus32 *host; const uint32_t *seed10; bool staged; ImageTexts say; };
    enum class ImageStep { IMAGE_HELD, STAGING_HELD, BODIES_UP, FILLED };
    template <class Hook>
    DeviceBuf<uint32_t> upload_image(const DevParams &dp, const uint32_t *tw, const ImageRows &r, Hook &&at);
    DeviceBuf<uint32_t> upload_twiddles(int N, const char *what);
    template <class Drop> void free_image(bool made, const char *what, Drop &&drop);
    template <class Src> size_t read_back(size_t words, Torus32 *out, size_t capacity, const char *what, Src &&src);
    // what run_unpack, run_inner, run_inner_sum, run_public_inner and run_public_sum_inner share (engine.cpp): the buffers and key-switch plans of `count` rows, then the chunks
    struct RowsPlan { int widest = 0, u_stride = 0; KsDesc *dks = nullptr; int32_t *u_buf = nullptr; KsLaunchPlan ks_wide, ks_last; };
    RowsPlan size_rows(const DeviceKeyImage *key, int u_stride, int count, bool to_slots);
    template <class MakeRows>
    void run_rows(const DeviceKeyImage *key, const RowsPlan &r, int count, size_t uw, SlotPool *pool, const int32_t *slots,
                  Torus32 *u_out, const char *what, MakeRows &&make_rows);
    void ensure_select_events();                        // kernel timing on: select_e0_ / select_e1_ exist from here on
    hipEvent_t select_e0_ = nullptr, select_e1_ = nullptr;
    bool select_timed_ = false;
    // what run_ring_rotate and run_ring_rotate_rows share (engine.cpp): the buffers of the operands, and their uploads
    struct RotateOperands { RingRotateArgs a; int32_t *dring = nullptr, *dindex = nullptr, *dslots = nullptr, *dlwe = nullptr; };
    RotateOperands size_ring_rotate(const DeviceKeyImage *key, int nring, bool ring_on_device, const int32_t *ring_index, SlotPool *pool,
                                    int count);
    void upload_ring_rotate(RotateOperands &o, const DeviceKeyImage *key, const Torus32 *ring, int nring, bool ring_on_device,
                            const int32_t *ring_index, SlotPool *pool, const int32_t *in_slots, const Torus32 *lwe_words, int count);
    // (behind everything else, as above) prepare_flush's key-switch plan of every (level, key) share of flight_plan_
    std::vector<KsLaunchPlan> flight_ks_plans_;
    // (likewise) the event pair last_ring_rotate_ms reads, made by the first timed rotation launch
    hipEvent_t rotate_e0_ = nullptr, rotate_e1_ = nullptr;
    bool rotate_timed_ = false;
};

}  // namespace tfhe_hip
