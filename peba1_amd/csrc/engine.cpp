// engine.cpp -- device memory, key upload and batched level execution.
#include "engine.hpp"

#include <algorithm>
#include <utility>
#include <vector>
#include <chrono>
#include <ctime>
#include <unistd.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>

#include "br_forms.hpp"
#include "ntt_field.hpp"

namespace tfhe_hip {

// ---- error channel ---------------------------------------------------------
static std::string g_last_error;
static std::mutex g_err_mtx;

void set_error(const std::string &msg) {
    std::lock_guard<std::mutex> g(g_err_mtx);
    g_last_error = msg;
}
const std::string &last_error_ref() { return g_last_error; }

[[noreturn]] void fatal(const std::string &msg) {
    set_error(msg);
    std::fprintf(stderr, "libtfhe-hip: fatal: %s\n", msg.c_str());
    std::abort();
}

[[noreturn]] void api_fail(const std::string &msg) { throw ApiError{msg}; }

void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) fatal(std::string(what) + ": " + hipGetErrorString(e));
}

// Device memory whose exhaustion is RECOVERABLE: the slot pool's growth, the per-flush scratch and
// the device image of a key (a server holds one per enrolled client's key set).
// A library living inside a matching server must not abort() because one request recorded more than the card holds:
// hipErrorOutOfMemory becomes an ApiError -- the call that needed the memory has no effect (the gates recorded so far
// stay recorded; a flush returns -1), tfhe_hip_last_error() says what could not be allocated, and the caller may free
// ciphertext arrays and go on.  Anything else hipMalloc can return is still fatal.  `g_alloc_cap` (test hook
// tfhe_hip_test_set_alloc_cap) makes allocations above a total fail the same way, so that the path has a test.
static long long g_alloc_cap = 0, g_alloc_total = 0;
void set_alloc_cap(long long bytes) { g_alloc_cap = bytes > 0 ? bytes : 0; }
long long alloc_held() { return g_alloc_total; }
void *recoverable_alloc(size_t bytes, const char *what) {
    void *p = nullptr;
    hipError_t e = hipErrorOutOfMemory;
    if (!(g_alloc_cap > 0 && g_alloc_total + (long long)bytes > g_alloc_cap)) e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();                 // the sticky error of the failed call must not fail the next launch check
        api_fail(std::string("out of device memory: ") + what + " needs " + std::to_string(bytes >> 20) + " MiB more (" +
                 std::to_string(g_alloc_total >> 20) + " MiB held by key images, the slot pool and the flush scratch); the call "
                 "had no effect -- free ciphertext arrays or key sets, flush less at a time, or lower TFHE_HIP_POOL_SLOTS");
    }
    hip_check(e, what);
    g_alloc_total += (long long)bytes;
    return p;
}
void recoverable_free(void *p, size_t bytes) {
    if (!p) return;
    (void)hipFree(p);
    g_alloc_total -= (long long)bytes;
}

// HIP's current device is per host thread and starts at 0: a worker thread of a multi-GPU server (rank r drives GPU r)
// that calls in without ever having selected a device -- or after selecting another one for its own work -- would launch
// on the engine's stream with the wrong device current.  Every method below that calls the HIP runtime therefore binds
// the calling thread to the engine's device for its duration and gives the caller's device back on return (ADVICE r4:
// a once-per-thread bind both changed the caller's device for good and missed a later hipSetDevice by the caller).
// The boots* recording calls never reach the runtime and pay nothing for this.
namespace {
class DeviceScope {
public:
    explicit DeviceScope(int want) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != want && hipSetDevice(want) == hipSuccess) prev_ = cur;
    }
    ~DeviceScope() { if (prev_ >= 0) (void)hipSetDevice(prev_); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
private:
    int prev_ = -1;
};
}  // namespace
#define ENGINE_DEVICE_SCOPE() DeviceScope device_scope_(Engine::get().device())

// ---- slot pool ---------------------------------------------------------------
// The pool is one contiguous device array (kernels index it by slot id) that starts small and doubles on demand up to
// `capacity` slots: a process that evaluates a few gates holds 0.2 GB, one that records whole matches grows to what its
// widest flush pins (5.3 GB were allocated up front whatever the caller did).
SlotPool::SlotPool(int ct_words, int ct_stride, size_t capacity) : words_(ct_words), stride_(ct_stride), max_cap_(capacity) {
    free_.reserve(std::min<size_t>(max_cap_, (size_t)1 << 17));
    grow(std::min<size_t>(max_cap_, (size_t)1 << 16));
}
SlotPool::~SlotPool() {
    ENGINE_DEVICE_SCOPE();
    recoverable_free(data_, cap_ * (size_t)stride_ * sizeof(int32_t));
}
void SlotPool::grow(size_t new_cap) {
    ENGINE_DEVICE_SCOPE();
    // (throws ApiError when the card is full: nothing has changed yet, the pool keeps its size and its contents)
    int32_t *fresh = static_cast<int32_t *>(recoverable_alloc(new_cap * (size_t)stride_ * sizeof(int32_t), "growing the ciphertext slot pool"));
    if (data_) {
        // growth happens while recording (host side).  A pipelined flush may still be in flight -- its launches carry
        // the old pointer -- and a caller's own stream may still read an exported buffer: wait for the whole device
        // once (every launch enqueued so far has then finished with the old buffer), copy, release
        Engine::get().sync_stream("sync before pool growth");      // bounded when a deadline is set (a collective may sit there)
        hip_check(hipDeviceSynchronize(), "sync before pool growth");
        hip_check(hipMemcpy(fresh, data_, cap_ * (size_t)stride_ * sizeof(int32_t), hipMemcpyDeviceToDevice), "copy slot pool");
        recoverable_free(data_, cap_ * (size_t)stride_ * sizeof(int32_t));
    }
    data_ = fresh;
    ref_.resize(new_cap, 0);
    level.resize(new_cap, 0);
    pending.resize(new_cap, 0);
    for (size_t i = new_cap; i-- > cap_;) free_.push_back((int32_t)i);
    cap_ = new_cap;
}
int32_t SlotPool::alloc() {
    if (free_.empty()) {
        if (cap_ >= max_cap_)
            api_fail("ciphertext slot pool exhausted (" + std::to_string(max_cap_) +
                     " slots); raise TFHE_HIP_POOL_SLOTS or free ciphertext arrays");
        grow(std::min(max_cap_, cap_ * 2));
    }
    const int32_t s = free_.back();
    free_.pop_back();
    ref_[s] = 1;
    level[s] = 0;
    pending[s] = 0;
    return s;
}
void SlotPool::release(int32_t s) {
    if (s < 0) return;
    if (--ref_[s] == 0) free_.push_back(s);
}

// ---- engine ------------------------------------------------------------------
Engine &Engine::get() {
    static Engine e;
    return e;
}

void Engine::set_device(int d) {
    if (inited_.load() && d != device_) fatal("tfhe_hip_set_device after the engine was initialised");
    device_ = d;
}

void Engine::ensure_init() {
    if (inited_.load(std::memory_order_acquire)) return;
    static std::mutex init_mtx;
    std::lock_guard<std::mutex> g(init_mtx);
    if (inited_.load(std::memory_order_relaxed)) return;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        fatal("no HIP device available: libtfhe-hip evaluates gates on the GPU only (there is no CPU fallback)");
    if (const char *env = std::getenv("TFHE_HIP_DEVICE")) device_ = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_KS_BLOCKS")) tunings.ks_target_blocks = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_KS_MAX_SPLITS")) tunings.ks_max_splits = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_KS_TILE")) tunings.ks_tile = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_KS_INDEX")) tunings.ks_index = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_KS_SPLIT_TIES")) tunings.ks_split_ties = std::atoi(env);
    DeviceScope bind(device_);               // (an invalid device shows at the first runtime call below)
    {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != device_) hip_check(hipSetDevice(device_), "hipSetDevice");
    }
    {
        hipDeviceProp_t prop;
        hip_check(hipGetDeviceProperties(&prop, device_), "hipGetDeviceProperties");
        cu_count_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    {
        int least = 0, greatest = 0;
        hip_check(hipDeviceGetStreamPriorityRange(&least, &greatest), "priority range");
        hip_check(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, greatest), "hipStreamCreate");
    }
    if (const char *env = std::getenv("TFHE_HIP_BR8_MAX")) tunings.br8_max_rotations = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_BR_TAIL8")) tunings.br_tail8 = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_BR_VARIANT")) tunings.br_variant = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_BR_TABLE")) tunings.br_digit_table = std::atoi(env);
    if (const char *env = std::getenv("TFHE_HIP_SYNC_DEADLINE_MS")) sync_deadline_ms = std::atoll(env);
    // a caller that cannot reach tfhe_hip_set_kernel_timing (the reference's unmodified program) asks for the per-level
    // times by naming the trace file
    if (std::getenv("TFHE_HIP_TRACE_TIMES")) kernel_timing = true;
    inited_.store(true, std::memory_order_release);
}

// ---- host waits ----------------------------------------------------------------
// Every host wait on the engine's stream goes through here.  Without a deadline it is hipStreamSynchronize.  With one
// (tuning "sync_deadline_ms" / TFHE_HIP_SYNC_DEADLINE_MS; libpeba1-dist sets it for communicators of more than one
// rank) the stream is polled, and a wait that outlasts the deadline -- a collective whose peer never arrived, a kernel
// that never ends -- prints what was waited for, by whom, and ends the process with TFHE_HIP_EXIT_DEADLINE: the job fails
// with a message instead of sitting in its scheduler's time limit.  No retry, no re-exec: the device state is unknown.
[[noreturn]] static void deadline_expired(const char *what, long long ms, const std::string &label) {
    std::fprintf(stderr, "libtfhe-hip: fatal: '%s' did not complete within %lld ms%s%s; the engine's stream is stuck behind a "
                         "collective or a kernel that does not finish -- exiting with code %d\n",
                 what, ms, label.empty() ? "" : " on ", label.c_str(), TFHE_HIP_EXIT_DEADLINE);
    std::fflush(stderr);
    _exit(TFHE_HIP_EXIT_DEADLINE);       // not exit(): runtime destructors would wait for the same stream
}

template <typename Query>
static void bounded_wait(Query &&query, const char *what, long long deadline_ms, const std::string &label) {
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        const hipError_t e = query();
        if (e == hipSuccess) return;
        if (e != hipErrorNotReady) hip_check(e, what);
        if ((spins & 63u) == 63u || spins > 4096u) {
            const long long ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
            if (ms >= deadline_ms) deadline_expired(what, deadline_ms, label);
        }
        if (spins > 4096u) {                 // a long wait: stop burning the core the recorder may want
            struct timespec ts = {0, 50 * 1000};
            nanosleep(&ts, nullptr);
        }
    }
}

void Engine::sync_stream(const char *what) {
    ENGINE_DEVICE_SCOPE();
    if (sync_deadline_ms <= 0) hip_check(hipStreamSynchronize(stream_), what);
    else bounded_wait([&] { return hipStreamQuery(stream_); }, what, sync_deadline_ms, diag_label);
    stage_.idle();                           // whatever was enqueued without a host wait has completed too
}

// a caller's own event (libpeba1-dist: the status words of a collective, on a stream of their own), bounded like every
// other host wait of the library.  Takes no engine state: safe beside a flush in flight.
void Engine::wait_event(hipEvent_t ev, const char *what, long long deadline_ms, const std::string &label) {
    ENGINE_DEVICE_SCOPE();
    if (deadline_ms <= 0) hip_check(hipEventSynchronize(ev), what);
    else bounded_wait([&] { return hipEventQuery(ev); }, what, deadline_ms, label);
}

bool Engine::pci_bus_id(char *out, int len) {
    ENGINE_DEVICE_SCOPE();
    return hipDeviceGetPCIBusId(out, len, device_) == hipSuccess;
}

// The pinned staging area (host_stage.hpp).  Host accesses of slot memory that do not go through the stream wait for its
// event too (sync_io; ADVICE r3: a decrypt of a sample imported behind an ncclGather read the slot before the scatter
// had written it): a transfer that returned without a host wait staged a list and left the event behind its launches.
void *HostStage::reserve(size_t bytes) {
    const StagePlace p = stage_place(pos_, capacity_, outstanding_, bytes);
    if (p.wait) wait();
    if (p.capacity != capacity_) {
        if (base_) hip_check(hipHostFree(base_), "free the pinned staging area");
        hip_check(hipHostMalloc(reinterpret_cast<void **>(&base_), p.capacity, hipHostMallocDefault), "the pinned staging area");
        capacity_ = p.capacity;
    }
    pos_ = p.next;
    outstanding_ = true, recorded_ = false;  // from here on, until a wait or a synchronised stream
    return base_ + p.offset;
}
void HostStage::uploaded() {
    if (!event_) hip_check(hipEventCreateWithFlags(&event_, hipEventDisableTiming), "staging event");
    hip_check(hipEventRecord(event_, owner_.stream()), "staging event record");
    outstanding_ = recorded_ = true;
}
void HostStage::wait() {
    ENGINE_DEVICE_SCOPE();
    if (!outstanding_) return;
    if (!recorded_) uploaded();              // (a call that failed behind its uploads left no event)
    owner_.wait_event(event_, "stream-ordered transfer", owner_.sync_deadline_ms, owner_.diag_label);
    outstanding_ = false;
}

void *Engine::scratch(Scratch idx, size_t bytes) {
    if (scratch_ptr_.size() <= idx) { scratch_ptr_.resize(idx + 1, nullptr); scratch_size_.resize(idx + 1, 0); }
    if (scratch_size_[idx] < bytes) {
        sync_stream("sync before scratch realloc");
        // the old buffer goes first (the two need not fit side by side); if the new one cannot be had the entry is empty,
        // which the next call sees as size 0 -- and the ApiError leaves the caller's call without effect
        recoverable_free(scratch_ptr_[idx], scratch_size_[idx]);
        scratch_ptr_[idx] = nullptr;
        scratch_size_[idx] = 0;
        size_t cap = bytes + bytes / 2 + 4096;
        try {
            scratch_ptr_[idx] = recoverable_alloc(cap, "the scratch buffers of a flush");
        } catch (const ApiError &) {
            if (cap == bytes + 4096) throw;
            cap = bytes + 4096;                  // without the growth margin
            scratch_ptr_[idx] = recoverable_alloc(cap, "the scratch buffers of a flush");
        }
        scratch_size_[idx] = cap;
    }
    return scratch_ptr_[idx];
}

static uint32_t bitrev32(uint32_t x, int bits) {
    uint32_t r = 0;
    for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1); x >>= 1; }
    return r;
}

// twiddles [prime][fwd,inv][N]: psi^{+-brv(i)} * R mod P, followed by the radix-4 quads
// [prime][fwd,inv][N/2][4]: entry e = 2^s + t (stage pair (s, s+1), block t) holds, with
// w1 = W[e], w2 = W[2e], w3 = W[2e+1]: {w2, w3, w1 w2, P - w1 w3}, all times R mod P
static std::vector<uint32_t> make_twiddles(int N) {
    int logn = 0;
    while ((1 << logn) < N) ++logn;
    std::vector<uint32_t> tw((size_t)24 * N);
    for (int q = 0; q < 2; ++q) {
        const uint64_t P = NTT_P[q];
        const uint64_t psi = powmod_c(NTT_GEN[q], (P - 1) / (uint64_t)(2 * N), P);
        const uint64_t ipsi = powmod_c(psi, P - 2, P);
        const uint64_t R = NTT_R[q];
        std::vector<uint64_t> plain[2] = {std::vector<uint64_t>(N), std::vector<uint64_t>(N)};
        uint64_t a = 1, b = 1;
        for (int i = 0; i < N; ++i) {
            const uint32_t j = bitrev32((uint32_t)i, logn);
            plain[0][j] = a;
            plain[1][j] = b;
            a = a * psi % P;
            b = b * ipsi % P;
        }
        for (int dir = 0; dir < 2; ++dir) {
            const std::vector<uint64_t> &W = plain[dir];
            uint32_t *t2 = &tw[(size_t)(q * 2 + dir) * N];
            uint32_t *t4 = &tw[(size_t)4 * N + (size_t)(q * 2 + dir) * 2 * N];
            for (int i = 0; i < N; ++i) t2[i] = (uint32_t)(W[i] * R % P);
            for (int e = 1; e < N / 2; ++e) {
                const uint64_t w1 = W[e], w2 = W[2 * e], w3 = W[2 * e + 1];
                t4[4 * e + 0] = (uint32_t)(w2 * R % P);
                t4[4 * e + 1] = (uint32_t)(w3 * R % P);
                t4[4 * e + 2] = (uint32_t)(w1 * w2 % P * R % P);
                t4[4 * e + 3] = (uint32_t)((P - w1 * w3 % P) % P * R % P);
            }
        }
        // Sub-transform tables of the split kernels (kernels.hip blind_rotate_split_kernel): after
        // stage 0 the two halves of the index range are independent N/2-point transforms whose stage
        // s' twiddle of block t' is W[(2 + h) 2^s' + t'].  Block h (6N words at 12N + 6N h) is laid
        // out exactly like the table of a stand-alone N/2-point transform, so the same code walks it.
        for (int h = 0; h < 2; ++h) {
            const int M = N / 2;
            uint32_t *blk = &tw[(size_t)12 * N + (size_t)h * 12 * M];
            for (int dir = 0; dir < 2; ++dir) {
                const std::vector<uint64_t> &W = plain[dir];
                uint32_t *t2 = blk + (size_t)(q * 2 + dir) * M;
                uint32_t *t4 = blk + (size_t)4 * M + (size_t)(q * 2 + dir) * 2 * M;
                auto full = [&](int e) {                 // e = 2^s' + t' -> (2 + h) 2^s' + t'
                    int top = 1;
                    while (top * 2 <= e) top *= 2;
                    return (2 + h) * top + (e - top);
                };
                t2[0] = 0;
                for (int e = 1; e < M; ++e) t2[e] = (uint32_t)(W[full(e)] * R % P);
                for (int e = 1; e < M / 2; ++e) {
                    const int f = full(e);
                    const uint64_t w1 = W[f], w2 = W[2 * f], w3 = W[2 * f + 1];
                    t4[4 * e + 0] = (uint32_t)(w2 * R % P);
                    t4[4 * e + 1] = (uint32_t)(w3 * R % P);
                    t4[4 * e + 2] = (uint32_t)(w1 * w2 % P * R % P);
                    t4[4 * e + 3] = (uint32_t)((P - w1 * w3 % P) % P * R % P);
                }
            }
        }
    }
    return tw;
}
// image scale: N^-1 (the inverse NTT is unscaled) times R (so that the
// Montgomery reduction of sum x*img leaves sum x*bk / N)
static void image_scale(int N, uint32_t scale_out[2]) {
    for (int q = 0; q < 2; ++q) scale_out[q] = (uint32_t)(powmod_c((uint64_t)N, NTT_P[q] - 2, NTT_P[q]) * NTT_R[q] % NTT_P[q]);
}
static ExpandSeed expand_seed(const uint32_t seed10[10]) {
    ExpandSeed seed;
    std::memcpy(seed.key, seed10, sizeof seed.key);
    seed.nonce[0] = seed10[8]; seed.nonce[1] = seed10[9];
    return seed;
}

static DevParams make_dev_params(const Params &p) {
    DevParams d;
    d.n = p.n; d.N = p.N; d.k = p.k; d.l = p.l; d.Bgbit = p.Bgbit; d.ks_t = p.ks_t; d.ks_basebit = p.ks_basebit;
    d.kpl = p.kpl(); d.ct_stride = p.ct_stride(); d.u_stride = p.u_stride();
    d.decomp_offset = p.decomp_offset(); d.ks_prec_offset = p.ks_prec_offset();
    d.mu = 1 << 29;
    d.br_variant = 0;
    d.digit_table = 1;
    d.clock_acc = nullptr;
    d.wg_times = nullptr;
    d.luts = nullptr;
    d.specs = nullptr;
    return d;
}

// why the kernels cannot evaluate gates under `p` exactly, or null.  Also applied by the file loaders (io.cpp).
const char *unsupported_reason(const Params &p) {
    if ((p.N != 1024 && p.N != 2048) || p.k != 1) return "the blind-rotate kernels are built for N = 1024 or 2048 and k = 1";
    if (p.n < 1 || p.n > 1024 || p.ct_stride() / 4 > 320) return "LWE dimension n must be in [1, 1024]";
    if (p.l < 1 || p.Bgbit < 1 || p.l * p.Bgbit > 32 || p.Bgbit > 12) return "gadget digits must fit 12 bits and l * Bgbit <= 32";
    if (p.ks_t < 1 || p.ks_basebit < 1 || p.ks_t * p.ks_basebit > 31 || p.ks_basebit > 8) return "key-switch digits out of range";
    // exactness of the CRT range: (k+1) l N (Bg/2) 2^31 must stay below P0*P1/2
    const double bound = (double)(p.k + 1) * p.l * p.N * (double)(1u << (p.Bgbit - 1)) * 2147483648.0;
    if (bound >= (double)CRT_EXACT_LIMIT) return "gadget parameters exceed the exact range of the two-prime NTT";
    // at least one kernel form must keep its lazy-arithmetic bounds for this (l, Bgbit) (br_forms.hpp)
    for (int f = 0; f < BR_FORM_COUNT; ++f)
        for (int t = 0; t < 3; ++t)
            if (br_form_admissible(f, p.N, p.l, p.Bgbit, t)) return nullptr;
    return "gadget (l, Bgbit) outside the exact range of every blind-rotate kernel form (br_forms.hpp)";
}

// ---- the upload path of the resident images ------------------------------------------------------------
// Every buffer of an image is a DeviceBuf: an ApiError out of any allocation (a card without room fails there, recoverably)
// gives back what the path holds so far as it unwinds -- the object is not made, tfhe_hip_last_error() says what was needed.
DeviceBuf<uint32_t> Engine::upload_twiddles(int N, const char *what) {
    const std::vector<uint32_t> host = make_twiddles(N);
    DeviceBuf<uint32_t> tw(host.size(), what);
    hip_check(hipMemcpy(tw.get(), host.data(), tw.bytes(), hipMemcpyHostToDevice), "upload twiddles");
    return tw;
}

// The NTT image of r.rows rows of r.polys polynomials under the tables `tw`: the image, the raw staging rows and, where
// seeded, the bodies are allocated before anything is enqueued; the staging rows are filled from the host or by
// launch_expand_bk (masks from the stream, bodies from the upload); launch_bk_transform follows, the stream is waited for
// and the staging goes with this scope.  at(step): where a cloud key allocates and enqueues what it has besides.
template <class Hook>
DeviceBuf<uint32_t> Engine::upload_image(const DevParams &dp, const uint32_t *tw, const ImageRows &r, Hook &&at) {
    const size_t body_words = (size_t)r.rows * dp.N, words = body_words * r.polys;
    uint32_t scale[2];
    image_scale(dp.N, scale);
    DeviceBuf<uint32_t> img(words * 2, r.say.img);
    at(ImageStep::IMAGE_HELD);
    DeviceBuf<int32_t> raw(words, r.say.raw), body;
    if (r.seed10) body = DeviceBuf<int32_t>(body_words, r.say.body);
    at(ImageStep::STAGING_HELD);
    if (!r.seed10) {
        hip_check(hipMemcpy(raw.get(), r.host, words * 4, hipMemcpyHostToDevice), r.say.upload);
    } else {
        if (r.staged) h2d_staged(body.get(), r.host, body_words, r.say.upload);
        else hip_check(hipMemcpy(body.get(), r.host, body_words * 4, hipMemcpyHostToDevice), r.say.upload);
        at(ImageStep::BODIES_UP);
        const ExpandBkArgs ea{expand_seed(r.seed10), r.rows, r.polys - 1, dp.N, body.get(), raw.get()};
        if (!launch_expand_bk(stream_, ea)) fatal(r.say.refused);
        hip_check(hipGetLastError(), (std::string(r.say.expand) + " launch").c_str());
    }
    at(ImageStep::FILLED);
    launch_bk_transform(stream_, dp, raw.get(), img.get(), tw, r.rows, r.polys, scale);
    hip_check(hipGetLastError(), (std::string(r.say.transform) + " launch").c_str());
    sync_stream(r.say.sync);
    return img;
}

// a resident image goes (drop()), if it was made: behind whatever on the stream still reads it
template <class Drop>
void Engine::free_image(bool made, const char *what, Drop &&drop) {
    ENGINE_DEVICE_SCOPE();
    if (!made) return;
    if (inited_) sync_stream(what);
    drop();
}

// what the two cloud-key forms share: the empty image of an accepted parameter set, and the kernels' view of the full one
static std::unique_ptr<DeviceKeyImage> new_key_image(const Params &p) {
    // a parameter set the kernels cannot run exactly is refused (the call that needed the key has no effect and
    // tfhe_hip_last_error() says why): a custom tuple or a loaded file may carry anything
    if (const char *why = unsupported_reason(p)) api_fail(why);
    auto img = std::make_unique<DeviceKeyImage>();
    img->dp = make_dev_params(p);
    fill_form_ok(img->form_ok, p.N, p.l, p.Bgbit);
    return img;
}
static DeviceKeyImage *finish_key_image(std::unique_ptr<DeviceKeyImage> img, size_t compact_rows) {
    img->key.bk_img = img->bk_img.get();
    img->key.ksk = img->ksk.get();
    img->key.ksk_zero = img->ksk.get() + compact_rows * img->dp.ct_stride;
    img->key.tw = img->tw.get();
    return img.release();
}

DeviceKeyImage *Engine::upload_key(const TfheHipCloudKey &ck) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const Params &p = ck.p;
    auto img = new_key_image(p);
    const int base = 1 << p.ks_basebit, stride = p.ct_stride();
    const size_t rows = (size_t)p.k * p.N * p.ks_t;
    // BK: upload raw, transform on device; the staging copy has gone when the compact KSK goes up
    img->tw = upload_twiddles(p.N, "the twiddle tables of a key");
    const ImageRows bk{p.n * p.kpl(), p.k + 1, ck.bk.data(), nullptr, false,
                       {"the bootstrapping-key image", "the staging copy of the bootstrapping key", nullptr, "upload bk", nullptr,
                        nullptr, "bk_transform", "bk_transform"}};
    img->bk_img = upload_image(img->dp, img->tw.get(), bk, [&](ImageStep s) {
        if (s == ImageStep::IMAGE_HELD) img->ksk = DeviceBuf<int32_t>((rows * (base - 1) + 1) * (size_t)stride, "the key-switching key");
    });

    // KSK: drop the all-zero digit-0 rows, pad rows to ct_stride
    std::vector<int32_t> compact((rows * (base - 1) + 1) * stride, 0);   // + one row of zeros (digit 0)
    for (size_t r = 0; r < rows; ++r)
        for (int v = 1; v < base; ++v)
            std::memcpy(&compact[(r * (base - 1) + (v - 1)) * stride], &ck.ksk[(r * base + v) * (size_t)(p.n + 1)],
                        (size_t)(p.n + 1) * 4);
    hip_check(hipMemcpy(img->ksk.get(), compact.data(), compact.size() * 4, hipMemcpyHostToDevice), "upload ksk");
    return finish_key_image(std::move(img), rows * (base - 1));
}

// ---- seed-compressed cloud keys (expand.hpp, expand.hip) ------------------------------------
DeviceKeyImage *Engine::upload_compressed_key(const TfheHipCloudKey &ck) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const Params &p = ck.p;
    auto img = new_key_image(p);
    const int stride = p.ct_stride();
    const size_t rows = p.ksk_body_words();                   // kN t (base-1) compact rows, and the zero row behind them
    DeviceBuf<int32_t> dksk;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    img->tw = upload_twiddles(p.N, "the twiddle tables of a key");
    const ImageRows bk{p.n * p.kpl(), p.k + 1, ck.bk_body.data(), ck.mask_seed.data(), false,
                       {"the bootstrapping-key image", "the staging copy of the bootstrapping key",
                        "the bodies of a compressed bootstrapping key", "upload bk bodies", "expand",
                        "expand: arguments outside what the kernels were built for", "bk_transform", "key expansion"}};
    // The compact KSK beside the image: its bodies go up, launch_expand_ksk writes it from the seed behind the BK's masks.
    // With upload_image's own steps the sequence is: allocate twiddles (above), BK image, [compact KSK], staging copy, BK
    // bodies, [KSK bodies]; upload BK bodies and [KSK bodies] (blocking); [event e0]; launch_expand_bk; [launch_expand_ksk;
    // event e1; clear the zero row]; launch_bk_transform; wait for the stream -- the bracketed steps are the hook's.  Only the
    // two expand launches lie between e0 and e1 (last_expand_ms).
    img->bk_img = upload_image(img->dp, img->tw.get(), bk, [&](ImageStep s) {
        if (s == ImageStep::IMAGE_HELD) {
            img->ksk = DeviceBuf<int32_t>((rows + 1) * (size_t)stride, "the key-switching key");
        } else if (s == ImageStep::STAGING_HELD) {
            dksk = DeviceBuf<int32_t>(rows, "the bodies of a compressed key-switching key");
        } else if (s == ImageStep::BODIES_UP) {
            hip_check(hipMemcpy(dksk.get(), ck.ksk_body.data(), dksk.bytes(), hipMemcpyHostToDevice), "upload ksk bodies");
            if (kernel_timing) {
                hip_check(hipEventCreate(&e0), "expand event");
                hip_check(hipEventCreate(&e1), "expand event");
                hip_check(hipEventRecord(e0, stream_), "expand event");
            }
        } else {
            const ExpandKskArgs ka{expand_seed(ck.mask_seed.data()), (uint64_t)(p.bk_mask_words() / 8), (int64_t)rows, p.n, stride,
                                   dksk.get(), img->ksk.get()};
            if (!launch_expand_ksk(stream_, ka)) fatal("expand: arguments outside what the kernels were built for");
            hip_check(hipGetLastError(), "expand launch");
            if (kernel_timing) hip_check(hipEventRecord(e1, stream_), "expand event");
            // the all-zero digit-0 row
            hip_check(hipMemsetAsync(img->ksk.get() + rows * stride, 0, (size_t)stride * 4, stream_), "clear the zero row");
        }
    });
    if (kernel_timing) {
        float ms = 0.f;
        hip_check(hipEventElapsedTime(&ms, e0, e1), "expand event");
        last_expand_ms = ms;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
    ++expand_stats.expanded_keys;
    expand_stats.expand_launches += 2;
    return finish_key_image(std::move(img), rows);
}

void Engine::run_expand_masks(const uint32_t seed10[10], int64_t first_word, int count, uint32_t *out) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    wait_flight();
    uint32_t *d = scratch_as<uint32_t>(S_EXPAND_WORDS, (size_t)count);
    if (!launch_expand_masks(stream_, expand_seed(seed10), first_word, count, d)) api_fail("expand_masks: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "expand_masks launch");
    ++expand_stats.expand_launches;
    d2h(out, d, (size_t)count, "download stream words");
    sync_stream("expand_masks");
}

// test paths: `words` device words copied back -- returns the word count, copies only if it fits `capacity`
// (src(): where they lie, asked for only once they are to be copied)
template <class Src>
size_t Engine::read_back(size_t words, Torus32 *out, size_t capacity, const char *what, Src &&src) {
    ENGINE_DEVICE_SCOPE();
    if (!out || capacity < words || !words) return words;
    wait_flight();
    hip_check(hipMemcpyAsync(out, src(), words * 4, hipMemcpyDeviceToHost, stream_), (std::string("download ") + what).c_str());
    sync_stream(what);
    return words;
}
size_t Engine::read_key_image(const DeviceKeyImage *img, int which, Torus32 *out, size_t capacity) {
    return which == 0 ? read_back(img->bk_img.bytes() / 4, out, capacity, "key image", [&] { return img->bk_img.get(); })
                      : read_back(img->ksk.bytes() / 4, out, capacity, "key image", [&] { return img->ksk.get(); });
}

void Engine::free_key(DeviceKeyImage *img) { free_image(img, "sync before key free", [&] { delete img; }); }

// ---- the byte-plane image of the matrix key switch (ks_matrix.hpp) --------------------------
static_assert(KS_MATRIX_SPAN == KSM_WAVES * KSM_CHUNK && KS_MATRIX_TILE == KSM_GATES, "launch_plan.hpp plans what ks_matrix.hip runs");
bool Engine::ensure_ks_planes(const DeviceKeyImage *key) {
    ENGINE_DEVICE_SCOPE();
    if (!key->ks_planes.empty()) return true;
    const DevParams &dp = key->dp;
    if (!ks_matrix_shape_ok(dp.k * dp.N, dp.ks_t, dp.ks_basebit)) return false;
    try {
        DeviceBuf<uint8_t> img(ks_matrix_image_bytes(dp.k * dp.N, dp.ct_stride), "the byte-plane image of a key-switching key");
        if (!launch_ksk_planes(stream_, dp, key->key, img.get())) return false;
        hip_check(hipGetLastError(), "ksk_planes launch");
        sync_stream("ksk_planes");
        key->ks_planes = std::move(img);
        return true;
    } catch (const ApiError &) {
        return false;                                    // the key works without the matrix form
    }
}

// ---- growable device tables -------------------------------------------------------
// `rows` rows of `words` words laid out at `stride` words a row (the rest of a row zero), and back
static std::vector<int32_t> pad_rows(const int32_t *src, size_t rows, size_t words, size_t stride) {
    std::vector<int32_t> padded(rows * stride, 0);
    for (size_t r = 0; r < rows; ++r) std::memcpy(&padded[r * stride], src + r * words, words * 4);
    return padded;
}
static void unpad_rows(int32_t *dst, const int32_t *src, size_t rows, size_t words, size_t stride) {
    for (size_t r = 0; r < rows; ++r) std::memcpy(dst + r * words, src + r * stride, words * 4);
}

// A device array of fixed-size entries that starts at 16 and doubles on demand; entries are handed out from a free list
// first.  The test polynomials and the extract specs of the caller's objects live in one each.
namespace {
struct DeviceTable {
    const size_t entry;                  // bytes
    const char *const grow_what, *const sync_what;
    char *dev = nullptr;
    size_t cap = 0, used = 0;            // entries allocated / ever handed out
    std::vector<int32_t> free;
    int32_t add(const void *src) {
        if (free.empty() && used == cap) {
            // (throws ApiError when the card is full: nothing has changed yet)
            const size_t fresh_cap = cap ? cap * 2 : 16;
            char *fresh = static_cast<char *>(recoverable_alloc(fresh_cap * entry, grow_what));
            if (dev) {
                // launches in flight carry the old pointer: wait for all of them, as the slot pool does when it grows
                Engine::get().sync_stream(sync_what);
                hip_check(hipDeviceSynchronize(), sync_what);
                hip_check(hipMemcpy(fresh, dev, cap * entry, hipMemcpyDeviceToDevice), grow_what);
                recoverable_free(dev, cap * entry);
            }
            dev = fresh;
            cap = fresh_cap;
        }
        int32_t index;
        if (!free.empty()) { index = free.back(); free.pop_back(); }
        else index = (int32_t)used++;
        // a blocking copy: no launch enqueued so far names this entry (new, or freed after its last op had run)
        hip_check(hipMemcpy(dev + (size_t)index * entry, src, entry, hipMemcpyHostToDevice), "upload a table entry");
        return index;
    }
    void release(int32_t index) { if (index >= 0 && (size_t)index < used) free.push_back(index); }
};
DeviceTable g_luts{(size_t)LUT_STRIDE * sizeof(int32_t), "growing the table of test polynomials", "sync before LUT table growth"};
DeviceTable g_specs{sizeof(ExtractSpec), "growing the table of extract specs", "sync before spec table growth"};
}  // namespace

int32_t Engine::lut_add(const Torus32 *words, int n_ring) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    if (n_ring < 1 || n_ring > LUT_STRIDE) api_fail("a test polynomial of more than " + std::to_string(LUT_STRIDE) + " words");
    return g_luts.add(pad_rows(words, 1, (size_t)n_ring, LUT_STRIDE).data());
}
void Engine::lut_free(int32_t index) { g_luts.release(index); }

int32_t Engine::spec_add(const ExtractSpec &xs) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    if (g_specs.free.empty() && g_specs.used == g_specs.cap && g_specs.cap > (size_t)XS_ENTRY_MASK / 2) api_fail("too many extract specs");
    const int32_t index = g_specs.add(&xs);
    if (spec_nout_.size() <= (size_t)index) spec_nout_.resize((size_t)index + 1, 0);
    spec_nout_[(size_t)index] = xs.nout;
    return index;
}
void Engine::spec_free(int32_t index) { g_specs.release(index); }

SlotPool *Engine::find_pool(const Params &p) const {
    for (SlotPool *pl : pools_)
        if (pl->ct_stride() == p.ct_stride() && pl->ct_words() == p.ct_words()) return pl;
    return nullptr;
}

SlotPool *Engine::pool_for(const Params &p) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    if (SlotPool *pl = find_pool(p)) return pl;
    // what the pool may GROW to (it starts at 65,536 slots and doubles on demand): 4,194,304 slots = 10.6 GB at n = 630 of
    // 288 GB of HBM -- eight 128-slot matches recorded while the eight of the flush in flight are still pinned
    size_t cap = 1u << 22;
    if (const char *env = std::getenv("TFHE_HIP_POOL_SLOTS")) cap = (size_t)std::atoll(env);
    if (cap < 8 || cap > MAX_POOL_SLOTS) {
        set_error("TFHE_HIP_POOL_SLOTS out of range [8, 2^29]; clamped");
        cap = cap < 8 ? 8 : MAX_POOL_SLOTS;
    }
    auto *pl = new SlotPool(p.ct_words(), p.ct_stride(), cap);
    // shared read-only slots: the trivial samples (0, -1/8) -- also what a fresh sample is -- and (0, +1/8)
    std::vector<Torus32> z(p.n, 0);
    pl->const_slot[0] = pl->alloc();
    write_slot(pl, pl->const_slot[0], z.data(), -(1 << 29));
    pl->const_slot[1] = pl->alloc();
    write_slot(pl, pl->const_slot[1], z.data(), 1 << 29);
    pools_.push_back(pl);
    return pl;
}

void Engine::write_slot(SlotPool *pool, int32_t slot, const Torus32 *a, Torus32 b) {
    ENGINE_DEVICE_SCOPE();
    // A blocking copy on the null stream is not ordered against the engine's non-blocking stream.  Slots a flush in
    // flight touches stay pinned, so a fresh slot is never one of those; but a slot freed right after a stream-ordered
    // export may still be waiting for its gather kernel: wait for such transfers, not for the whole stream
    // (a pipelined flush keeps running under the recording that calls this).
    sync_io();
    std::vector<int32_t> tmp(pool->ct_stride(), 0);
    std::memcpy(tmp.data(), a, (size_t)(pool->ct_words() - 1) * 4);
    tmp[pool->ct_words() - 1] = b;
    hip_check(hipMemcpy(pool->data() + (size_t)slot * pool->ct_stride(), tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice),
              "write_slot");
}

void Engine::read_slot(SlotPool *pool, int32_t slot, Torus32 *a, Torus32 *b) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();
    // on the engine's stream, then waited for: ordered behind everything enqueued there -- a flush, and a stream-ordered
    // import that nobody waited for (the scatter behind an ncclGather of tfhe_hip_import_samples_device_async)
    std::vector<int32_t> tmp(pool->ct_stride());
    d2h(tmp.data(), pool->data() + (size_t)slot * pool->ct_stride(), tmp.size(), "read_slot");
    sync_stream("read_slot");
    std::memcpy(a, tmp.data(), (size_t)(pool->ct_words() - 1) * 4);
    *b = tmp[pool->ct_words() - 1];
}

// The slot list goes up through the pinned staging area, so that the stream-ordered (no host wait) forms never read
// host memory the caller has already released.
void Engine::write_slots_packed(SlotPool *pool, const int32_t *slots, int count, const Torus32 *words, bool on_device, bool wait) {
    ENGINE_DEVICE_SCOPE();
    if (count <= 0) return;
    if (count > MAX_PACKED_SAMPLES) api_fail("too many samples in one packed transfer");
    const size_t nwords = (size_t)count * pool->ct_words();
    int32_t *dslots = scratch_as<int32_t>(S_SLOTS, (size_t)count);
    h2d_staged(dslots, slots, (size_t)count, "upload slot list");
    const int32_t *src = on_device ? words : scratch_upload(S_WORDS, words, nwords, "upload packed words");
    launch_scatter_slots(stream_, pool->data(), pool->ct_stride(), pool->ct_words(), dslots, count, src);
    finish(wait || !on_device, "scatter slots");             // (a host source is the caller's pageable memory)
}

void Engine::read_slots_packed(SlotPool *pool, const int32_t *slots, int count, Torus32 *words, bool on_device, bool wait) {
    ENGINE_DEVICE_SCOPE();
    if (count <= 0) return;
    if (count > MAX_PACKED_SAMPLES) api_fail("too many samples in one packed transfer");
    const size_t nwords = (size_t)count * pool->ct_words();
    // (a list in flight from an earlier stream-ordered call is read by its kernel before this copy lands: one stream)
    int32_t *dslots = scratch_as<int32_t>(S_SLOTS, (size_t)count);
    h2d_staged(dslots, slots, (size_t)count, "upload slot list");
    int32_t *dst = on_device ? words : scratch_as<int32_t>(S_WORDS, nwords);
    launch_gather_slots(stream_, pool->data(), pool->ct_stride(), pool->ct_words(), dslots, count, dst);
    if (!on_device) d2h(words, dst, nwords, "download packed words");
    finish(wait || !on_device, "gather slots");              // (a host destination has its words on return)
}

hipEvent_t Engine::next_timing_event() {
    if (timing_used_ == timing_events_.size()) {
        hipEvent_t e;
        hip_check(hipEventCreate(&e), "timing event");
        timing_events_.push_back(e);
    }
    return timing_events_[timing_used_++];
}

BrPlan Engine::plan_br_launch(const DeviceKeyImage *key, int count, bool acc_dump) const {
    const BrPlan plan = plan_br(key->form_ok, key->dp.N, key->dp.l, tunings, cu_count_, count, wg_times_dbg_ != nullptr, acc_dump);
    if (plan.form < 0) fatal("no admissible blind-rotate form (upload_key should have refused this key)");
    return plan;
}

void Engine::launch_br(const DeviceKeyImage *key, const BrPlan &plan, const BrLaunch &a) {
    ENGINE_DEVICE_SCOPE();
    const hipStream_t stream = a.stream ? a.stream : stream_;
    const int form = plan.form, head = a.count - plan.tail;
    if (a.mk_keys && form != BR_FORM_WIDE4 && form != BR_FORM_WAVE8) fatal("launch_br: no multi-key kernel for this form");
    if (plan.tail && (form != BR_FORM_WIDE4 || a.acc_dbg)) fatal("launch_br: a tail behind a launch that cannot be split");
    DevParams dp = key->dp;
    dp.digit_table = plan.tables;
    dp.luts = a.luts ? a.luts : reinterpret_cast<const int32_t *>(g_luts.dev);
    dp.specs = a.specs ? a.specs : reinterpret_cast<const ExtractSpec *>(g_specs.dev);
    // per-form and per-table-mode launch counters (TfheHipStats): what ran, whatever the tunings asked for
    auto note = [&](int f) {
        ++(f == BR_FORM_WIDE4 ? stats.br_wide4_launches : f == BR_FORM_SPLIT ? stats.br_split_launches
           : f == BR_FORM_WAVE8 ? stats.br_wave8_launches : stats.br_wave2_launches);
        // (the mode the launchers run, not the one planned: a gadget whose digits cannot index the tables multiplies)
        const int ran = br_tables_run(f, dp.l, dp.Bgbit, plan.tables);
        ++(ran == 0 ? stats.br_tables0_launches : ran == 1 ? stats.br_tables1_launches : stats.br_tables2_launches);
    };
    if (kernel_timing) {
        if (!clock_acc_) {
            hip_check(hipMalloc(&clock_acc_, 2 * sizeof(unsigned long long)), "hipMalloc(clock sums)");
            hip_check(hipMemset(clock_acc_, 0, 2 * sizeof(unsigned long long)), "hipMemset(clock sums)");
        }
        dp.clock_acc = clock_acc_;
    }
    if (form == BR_FORM_WIDE4 || form == BR_FORM_WAVE8) dp.wg_times = wg_times_dbg_;
    note(form);
    if (form == BR_FORM_WAVE2) launch_blind_rotate2(stream, dp, key->key, a.pool, a.rots, a.count, a.u_buf, a.acc_dbg);
    else if (form == BR_FORM_SPLIT) launch_blind_rotate_split(stream, dp, key->key, a.pool, a.rots, a.count, a.u_buf, a.acc_dbg);
    else if (form == BR_FORM_WAVE8 && a.mk_keys) launch_blind_rotate8_mk(stream, dp, key->key, a.mk_keys, a.mk_rot_keys, a.pool, a.rots, a.count, a.u_buf);
    else if (form == BR_FORM_WAVE8) launch_blind_rotate8(stream, dp, key->key, a.pool, a.rots, a.count, a.u_buf, a.acc_dbg);
    else if (a.mk_keys) launch_blind_rotate4_mk(stream, dp, key->key, a.mk_keys, a.mk_rot_keys, a.pool, a.rots, head, a.u_buf);
    else launch_blind_rotate4(stream, dp, key->key, a.pool, a.rots, head, a.u_buf, a.acc_dbg);
    if (!plan.tail) return;
    // the last round on the 8-wave form, with the event between the two launches where the caller has a reader for it
    if (a.mid) { *a.mid = next_timing_event(); hip_check(hipEventRecord(*a.mid, stream), "event"); }
    note(BR_FORM_WAVE8);
    if (a.mk_keys) launch_blind_rotate8_mk(stream, dp, key->key, a.mk_keys, a.mk_rot_keys + head, a.pool, a.rots + head, plan.tail, a.u_buf);
    else launch_blind_rotate8(stream, dp, key->key, a.pool, a.rots + head, plan.tail, a.u_buf, nullptr);
}

KsLaunchPlan Engine::plan_ks_launch(const DeviceKeyImage *key, int count, bool has_image) const {
    const DevParams &dp = key->dp;
    return tfhe_hip::plan_ks_launch(tunings, cu_count_, count, KsShape{dp.k * dp.N, dp.ks_t, dp.ks_basebit, dp.ct_stride}, has_image);
}

void Engine::launch_ks(const DeviceKeyImage *key, const KsLaunchPlan &plan, const int32_t *u_buf, const KsDesc *descs,
                       int32_t *pool, hipStream_t stream) {
    ENGINE_DEVICE_SCOPE();
    if (!stream) stream = stream_;
    const DevParams &dp = key->dp;
    // the buffer as whoever built the plan sized it from partial_bytes, before anything was enqueued: it never grows here
    int32_t *partial = static_cast<int32_t *>(scratch(S_KS_PARTIAL, 0));
    if (plan.partial_bytes > scratch_size_[S_KS_PARTIAL]) fatal("launch_ks: the plan's partial sums do not fit their buffer");
    for (int i = 0, done = 0; i < plan.parts; done += plan.gates(i++)) {
        const KsPlan &part = plan.part(i);                   // (the counters say what ran, part by part)
        if (part.form == KS_FORM_MATRIX) {
            ++ks_matrix_stats.ks_matrix_launches;
            if (key->ks_planes.empty() || !launch_keyswitch_matrix(stream, dp, key->ks_planes.get(), u_buf, descs + done, plan.gates(i), pool))
                fatal("launch_ks: the planned matrix key switch has no kernel for this shape");
            continue;
        }
        ++(part.form == KS_FORM_INDEX ? stats.ks_index_launches : part.form == KS_FORM_STRIP ? stats.ks_strip_launches
                                                                                             : stats.ks_pergate_launches);
        if (!launch_keyswitch(stream, dp, key->key, u_buf, descs + done, plan.gates(i), pool, part.splits,
                              part.splits > 1 ? partial : nullptr, part.tile, part.form != KS_FORM_STRIP))
            fatal("launch_ks: the planned key-switch form has no kernel instantiation");
    }
}

// Step one of a flush, and the only one that can throw or fatal() on a bad plan: the checks of the plan and the sizing of
// every device buffer the flush uses.  scratch() may reallocate, which must not happen under a running launch -- and it
// may throw (out of device memory: recoverable_alloc), in which case nothing has been enqueued, the plan is still the
// caller's, its recorded gates are still pending and its flush returns -1 (recorder.cpp flush_locked releases nothing of
// the flush before execute() returns).
Engine::FlushBuffers Engine::prepare_flush(const std::vector<const DeviceKeyImage *> &keys, LevelPlan &plan) {
    // several keys (recorder "batch_keys"): all of one parameter set, so the descriptors, the extract buffer, the twiddles
    // and the form rules are those of keys[0]; each rotation and each key switch runs under its own gate's key
    const DeviceKeyImage *key = keys.at(0);
    const int nkeys = plan.nkeys;
    if (nkeys < 1 || (size_t)nkeys != keys.size()) fatal("execute: the plan's key count differs from the flush's key list");
    // (recorder.cpp select_key keeps keys of another set out of a recording; checked again here, before any launch, because
    // a key with a larger ring or gadget than keys[0]'s would be read beyond its image and write beyond the extract buffer)
    for (const DeviceKeyImage *k : keys) {
        const DevParams &a = key->dp, &b = k->dp;
        if (a.n != b.n || a.N != b.N || a.k != b.k || a.l != b.l || a.Bgbit != b.Bgbit || a.ks_t != b.ks_t ||
            a.ks_basebit != b.ks_basebit)
            fatal("execute: the keys of a multi-key flush differ in a parameter that evaluation reads");
    }
    FlushBuffers fb{};
    fb.rots = scratch_as<RotDesc>(S_ROTS, plan.rots.size(), 16);
    fb.ks = scratch_as<KsDesc>(S_KS, plan.kss.size(), 16);
    fb.nots = scratch_as<NotDesc>(S_NOTS, plan.nots.size(), 16);
    if (!plan.lins.empty()) {
        // (every launch range lies inside the descriptors, every descriptor inside its own arrays and inside the pool)
        if (plan.lin_level_off.size() != (size_t)plan.levels + 2 || plan.lin_launch_off.empty() ||
            (size_t)plan.lin_level_off.back() + 1 != plan.lin_launch_off.size() || (size_t)plan.lin_launch_off.back() != plan.lins.size())
            fatal("execute: the launch ranges of the linear combinations do not cover their descriptors");
        for (const LinDesc &d : plan.lins) {
            if (d.nin < 1 || d.nin > LIN_DESC_MAX_IN || d.dst_slot < 0) fatal("execute: a malformed linear combination");
            for (int t = 0; t < d.nin; ++t)
                if (d.slot[t] < 0 || d.slot[t] == d.dst_slot) fatal("execute: a linear combination reads a slot it may not");
        }
        fb.lins = scratch_as<LinDesc>(S_LINS, plan.lins.size());
    }
    // extract buffer, sized for the widest level, and the key-switch plans that run_level runs, with their partial sums
    fb.u_buf = scratch_as<int32_t>(S_EXTRACT, (size_t)(std::max(plan.max_rots, plan.max_extracts) + 1) * key->dp.u_stride);
    size_t partial = 0;
    const std::vector<int32_t> &ks_shares = nkeys == 1 ? plan.ks_off : plan.ks_koff;   // one key-switch launch per (level, key)
    flight_ks_plans_.clear();
    for (size_t sg = 0; sg + 1 < ks_shares.size(); ++sg) {
        // a launch wide enough for the matrix form: its key gets the byte-plane image now, before anything is enqueued (a
        // card without room for it: the launch is planned again without, and runs and is sized as that plan says)
        const DeviceKeyImage *share_key = keys[nkeys == 1 ? 0 : sg % (size_t)nkeys];
        const int width = ks_shares[sg + 1] - ks_shares[sg];
        KsLaunchPlan kp = plan_ks_launch(share_key, width, true);
        if (kp.full.form == KS_FORM_MATRIX && !ensure_ks_planes(share_key)) kp = plan_ks_launch(share_key, width, false);
        partial = std::max(partial, kp.partial_bytes);
        flight_ks_plans_.push_back(kp);
    }
    (void)scratch(S_KS_PARTIAL, partial);
    // the key table and the key index of every rotation
    if (nkeys > 1) {
        fb.keys = scratch_as<DevKey>(S_KEYS, (size_t)nkeys);
        fb.rot_keys = scratch_as<int32_t>(S_ROT_KEYS, plan.rot_key.size(), 16);
        plan.dev_keys.resize((size_t)nkeys);
        for (int k = 0; k < nkeys; ++k) plan.dev_keys[(size_t)k] = keys[(size_t)k]->key;
    }
    // every table entry a rotation names is the engine's, and every output of a multi-output rotation lies inside the
    // extract buffer sized above
    uint64_t lut_rots = 0, multi_rots = 0, multi_outs = 0;
    for (const RotDesc &rd : plan.rots) {
        if (rd.lut >= 0) {
            if ((size_t)rd.lut >= g_luts.used) fatal("execute: a rotation names a test polynomial the engine does not hold");
            ++lut_rots;
        }
        if (rd.spec >= 0) {
            if ((size_t)(rd.spec & XS_ENTRY_MASK) >= g_specs.used) fatal("execute: a rotation names an extract spec the engine does not hold");
            if (rd.u_index < 0 || rd.u_index + spec_nout_[(size_t)(rd.spec & XS_ENTRY_MASK)] > plan.max_extracts)
                fatal("execute: a multi-output rotation writes beyond the extract buffer");
            ++multi_rots;
            multi_outs += (uint64_t)__builtin_popcount((unsigned)(rd.spec >> XS_WANTED_SHIFT));
        }
    }
    stats.lut_rotations += lut_rots;
    stats.multi_rotations += multi_rots;
    stats.multi_outputs += multi_outs;
    return fb;
}

// Step two: the plan changes hands and its descriptors and key table go to the device.
void Engine::upload_flush(const FlushBuffers &fb, LevelPlan &&plan_in) {
    flight_plan_ = std::move(plan_in);               // owns the host descriptors until the uploads have certainly happened
    const LevelPlan &plan = flight_plan_;
    if (!plan.rots.empty()) h2d(fb.rots, plan.rots.data(), plan.rots.size(), "upload rots");
    if (!plan.kss.empty()) h2d(fb.ks, plan.kss.data(), plan.kss.size(), "upload ks");
    if (!plan.nots.empty()) h2d(fb.nots, plan.nots.data(), plan.nots.size(), "upload nots");
    if (!plan.lins.empty()) h2d(fb.lins, plan.lins.data(), plan.lins.size(), "upload lins");
    if (plan.nkeys > 1) {
        h2d(fb.keys, plan.dev_keys.data(), plan.dev_keys.size(), "upload keys");
        if (!plan.rot_key.empty()) h2d(fb.rot_keys, plan.rot_key.data(), plan.rot_key.size(), "upload rot keys");
    }
}

// Step three, once per level L of flight_plan_ (0: the linear ops riding on the inputs): the blind rotations, the key switches,
// the NOTs and then, rank by rank, the linear combinations of the level.  shared_end: the previous level's end event where it
// can serve as this level's start.
void Engine::run_level(const std::vector<const DeviceKeyImage *> &keys, SlotPool *pool, const FlushBuffers &fb, int L, hipEvent_t &shared_end) {
    const LevelPlan &plan = flight_plan_;
    const DeviceKeyImage *key = keys[0];
    const int nkeys = plan.nkeys;
    const size_t gg = L > 0 ? (size_t)(L - 1) : 0;       // gate index
    const int nrot = L > 0 ? plan.rot_off[gg + 1] - plan.rot_off[gg] : 0;
    const int nks = L > 0 ? plan.ks_off[gg + 1] - plan.ks_off[gg] : 0;
    const int nnot = plan.not_off[(size_t)L + 1] - plan.not_off[(size_t)L];
    const int lin0 = plan.lins.empty() ? 0 : plan.lin_level_off[(size_t)L], lin1 = plan.lins.empty() ? 0 : plan.lin_level_off[(size_t)L + 1];
    if (nrot == 0 && nks == 0 && nnot == 0 && lin0 == lin1) return;
    Timed t{nullptr, nullptr, nullptr, false, nrot};
    // a level's start event is the previous level's end event where nothing was enqueued in between (no NOT launch
    // behind the key switch): two events per level instead of three -- an event costs the stream a few
    // microseconds, 1,131 of them 4-15 ms of a match
    if (kernel_timing) {
        if (shared_end) t.e0 = shared_end;
        else { t.e0 = next_timing_event(); hip_check(hipEventRecord(t.e0, stream_), "event"); }
        shared_end = nullptr;
    }
    if (nrot) {
        // one plan per level, from its total width; the statistics follow from the plan and the launches made
        const BrPlan bp = plan_br_launch(key, nrot, false);
        int launches = 0;
        BrLaunch a{pool->data(), fb.rots + plan.rot_off[gg], nrot, fb.u_buf, nullptr, stream_};
        if (nkeys == 1 || bp.form == BR_FORM_WIDE4 || bp.form == BR_FORM_WAVE8) {
            // one launch, two with a tail; several keys: each rotation under its own key through the key table
            a.mk_keys = fb.keys;
            a.mk_rot_keys = fb.keys ? fb.rot_keys + plan.rot_off[gg] : nullptr;
            a.mid = kernel_timing ? &t.em : nullptr;
            launch_br(key, bp, a);
            launches = bp.tail ? 2 : 1;
        } else {
            // no multi-key kernel for this form: one launch of it per key over that key's contiguous run of the
            // level's rotations (bp.tail is 0: only the 4-wave form has one)
            for (int k = 0; k < nkeys; ++k) {
                const size_t sg = gg * (size_t)nkeys + (size_t)k;
                a.rots = fb.rots + plan.rot_koff[sg];
                a.count = plan.rot_koff[sg + 1] - plan.rot_koff[sg];
                if (!a.count) continue;
                launch_br(keys[(size_t)k], bp, a);
                ++launches;
            }
        }
        t.wide8 = bp.form == BR_FORM_WAVE8;
        t.tail = bp.tail;
        stats.br_launches += (uint64_t)launches;
        if (t.wide8 || t.tail) { ++stats.br8_launches; stats.br8_rotations += (uint64_t)(t.wide8 ? nrot : t.tail); }
    }
    if (kernel_timing) { t.e1 = next_timing_event(); hip_check(hipEventRecord(t.e1, stream_), "event"); }
    // the key-switch kernels are single-key: one launch per key with a share of the level, by the plan prepare_flush made of
    // it (an empty share: a plan of no parts)
    for (int k = 0; k < nkeys && nks; ++k) {
        const size_t sg = gg * (size_t)nkeys + (size_t)k;
        const int32_t first = nkeys == 1 ? plan.ks_off[gg] : plan.ks_koff[sg];
        launch_ks(keys[(size_t)k], flight_ks_plans_[sg], fb.u_buf, fb.ks + first, pool->data(), stream_);
    }
    if (kernel_timing) {
        t.e2 = next_timing_event(); hip_check(hipEventRecord(t.e2, stream_), "event"); flight_timed_.push_back(t);
        if (nnot == 0 && lin0 == lin1) shared_end = t.e2;
    }
    launch_not(stream_, key->dp, fb.nots + plan.not_off[(size_t)L], nnot, pool->data());
    // a rank reads what the ranks before it wrote: one launch each, in stream order
    for (int j = lin0; j < lin1; ++j) {
        const int first = plan.lin_launch_off[(size_t)j], n = plan.lin_launch_off[(size_t)j + 1] - first;
        launch_linear(stream_, key->dp, fb.lins + first, n, pool->data());
        stats.linear_ops += (uint64_t)n;
        stats.lincomb_ops += (uint64_t)n;
        ++stats.lincomb_launches;
    }
    stats.blind_rotates += (uint64_t)nrot;
    stats.keyswitches += (uint64_t)nks;
    stats.linear_ops += (uint64_t)nnot;
}

// wait = false: the launches are enqueued and the call returns; the flush is "in flight" until wait_flight() (called by
// the next execute() before it touches the descriptor buffers, by every host read of a slot, by the statistics).  The
// host work of the NEXT flush -- recording, dead-gate elimination, levelling, building its plan -- then overlaps this
// one's execution (recorder.cpp flush_locked).
void Engine::execute(const std::vector<const DeviceKeyImage *> &keys, SlotPool *pool, LevelPlan &&plan_in, bool wait) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();                                   // at most one flush in flight: its descriptors and scratch are in use
    flight_t0_ = std::chrono::steady_clock::now();
    const FlushBuffers fb = prepare_flush(keys, plan_in);
    upload_flush(fb, std::move(plan_in));
    const int levels = flight_plan_.levels;
    last_flush_keys = flight_plan_.nkeys;
    timing_used_ = 0;                                // timing events used: base, then 2-3 (one more with a tail launch) per level
    flight_timed_.clear();
    flight_base_ = nullptr;
    if (kernel_timing) {
        flight_base_ = next_timing_event();
        hip_check(hipEventRecord(flight_base_, stream_), "event");
        flight_timed_.reserve((size_t)levels + 1);
    }
    hipEvent_t shared_end = nullptr;
    for (int L = 0; L <= levels; ++L) run_level(keys, pool, fb, L, shared_end);
    if (const char *trace = std::getenv("TFHE_HIP_TRACE_LEVELS")) {   // diagnostic: rotations per level
        if (FILE *f = std::fopen(trace, "a")) {
            std::fprintf(f, "flush levels=%d lanes=1\n", levels);
            for (int L = 1; L <= levels; ++L)
                std::fprintf(f, "%d 0 %d\n", L, flight_plan_.rot_off[(size_t)L] - flight_plan_.rot_off[(size_t)L - 1]);
            std::fclose(f);
        }
    }
    hip_check(hipGetLastError(), "kernel launch");
    flight_levels_ = levels;
    in_flight_ = true;
    if (wait) wait_flight();
}

void Engine::wait_flight() {
    ENGINE_DEVICE_SCOPE();
    if (!in_flight_) return;
    in_flight_ = false;
    const int levels = flight_levels_;
    std::vector<Timed> &timed = flight_timed_;
    hipEvent_t base = flight_base_;
    sync_stream("level execution");
    if (kernel_timing && base) {
        // durations per launch, and the union of the blind-rotate intervals
        std::vector<std::pair<float, float>> br;
        br.reserve(timed.size());
        // diagnostic: start, blind-rotate and key-switch time of every level (TFHE_HIP_TRACE_TIMES = file)
        FILE *tf = nullptr;
        if (const char *trace = std::getenv("TFHE_HIP_TRACE_TIMES")) tf = std::fopen(trace, "a");
        // "flush levels=L start_ms=S": S = host time of the flush's start since the process's first flush (the gaps between
        // flushes are the caller's own time: recording, encrypting, decrypting)
        static const auto trace_t0 = flight_t0_;
        if (tf) std::fprintf(tf, "flush levels=%d start_ms=%.3f\n", levels,
                             std::chrono::duration<double, std::milli>(flight_t0_ - trace_t0).count());
        for (const Timed &t : timed) {
            float a = 0, b = 0, c = 0;
            hip_check(hipEventElapsedTime(&a, base, t.e0), "elapsed");
            hip_check(hipEventElapsedTime(&b, base, t.e1), "elapsed");
            hip_check(hipEventElapsedTime(&c, base, t.e2), "elapsed");
            if (tf) std::fprintf(tf, "%d %.4f %.4f %.4f %d\n", t.nrot, a, b - a, c - b, t.wide8 ? 1 : 0);
            stats.ms_blind_rotate += b - a;
            if (t.wide8) stats.ms_blind_rotate8 += b - a;
            if (t.em) {
                float m = 0;
                hip_check(hipEventElapsedTime(&m, base, t.em), "elapsed");
                stats.ms_blind_rotate8 += b - m;
            }
            stats.ms_keyswitch += c - b;
            if (b > a) br.emplace_back(a, b);
        }
        std::sort(br.begin(), br.end());
        float cur_a = 0, cur_b = -1;
        for (const auto &iv : br) {
            if (cur_b < cur_a || iv.first > cur_b) {
                if (cur_b >= cur_a) stats.ms_blind_rotate_busy += cur_b - cur_a;
                cur_a = iv.first; cur_b = iv.second;
            } else {
                cur_b = std::max(cur_b, iv.second);
            }
        }
        if (cur_b >= cur_a) stats.ms_blind_rotate_busy += cur_b - cur_a;
        if (tf) {
            std::fprintf(tf, "wall_ms=%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - flight_t0_).count());
            std::fclose(tf);
        }
    }
    if (kernel_timing && clock_acc_) {
        unsigned long long sums[2] = {0, 0};
        hip_check(hipMemcpy(sums, clock_acc_, sizeof sums, hipMemcpyDeviceToHost), "read clock sums");
        hip_check(hipMemset(clock_acc_, 0, sizeof sums), "clear clock sums");
        stats.clk_shader_cycles += sums[0];
        stats.clk_ref_ticks += sums[1];
    }
    stats.levels += (uint64_t)levels;
    ++stats.flushes;
    stats.ms_flush_wall += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - flight_t0_).count();
    timed.clear();
    flight_plan_ = LevelPlan{};
}

void Engine::run_raw_rotations(const DeviceKeyImage *key, const Torus32 *lin, int count, const int32_t *lut_index,
                               const Torus32 *polys, int npolys, const int32_t *spec_index, const ExtractSpec *specs, int nspecs,
                               int out_rows, Torus32 *u_out, Torus32 *acc_out, const char *name) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();
    const DevParams &dp = key->dp;
    const std::string who = std::string(name) + ": ";
    for (int c = 0; c < count; ++c) {
        if (lut_index && lut_index[c] >= npolys) api_fail(who + "a LUT index beyond the table");
        if (spec_index && spec_index[c] >= nspecs) api_fail(who + "a spec index beyond the table");
    }
    for (int t = 0; t < nspecs; ++t)
        if (const char *why = extract_spec_error(specs[t], dp.N)) api_fail(who + why);
    // the call's own tables, laid out like the engine's (without one: the engine's, which no descriptor here names)
    BrLaunch a{};
    const std::vector<int32_t> table = lut_index ? pad_rows(polys, (size_t)npolys, (size_t)dp.N, LUT_STRIDE) : std::vector<int32_t>();
    if (lut_index) a.luts = scratch_upload(S_RAW_LUTS, table.data(), table.size(), "upload LUTs");
    if (spec_index) a.specs = scratch_upload(S_RAW_SPECS, specs, (size_t)nspecs, "upload specs");
    // temporary "pool": count slots holding lin
    const std::vector<int32_t> padded = pad_rows(lin, (size_t)count, (size_t)dp.n + 1, (size_t)dp.ct_stride);
    a.pool = scratch_upload(S_RAW_POOL, padded.data(), padded.size(), "upload lin");
    // u_index: the outputs of the combinations before this one (a combination without a spec has one)
    std::vector<RotDesc> rots(count);
    int32_t total = 0;
    for (int c = 0; c < count; ++c) {
        rots[c] = RotDesc{c, c, 1, 0, 0, total};
        if (lut_index && lut_index[c] >= 0) { rots[c].lut = lut_index[c]; ++stats.lut_rotations; }
        int nout = 1;
        if (spec_index && spec_index[c] >= 0) {
            nout = specs[spec_index[c]].nout;
            rots[c].spec = spec_index[c] | ((1 << nout) - 1) << XS_WANTED_SHIFT;
            ++stats.multi_rotations;
            stats.multi_outputs += (uint64_t)nout;
        }
        total += nout;
    }
    a.rots = scratch_upload(S_ROTS, rots.data(), rots.size(), "upload rots");
    a.count = count;
    a.u_buf = scratch_as<int32_t>(S_EXTRACT, (size_t)(total + 1) * dp.u_stride);
    a.acc_dbg = acc_out ? scratch_as<int32_t>(S_RAW_ACC, (size_t)count * 2 * dp.N) : nullptr;
    launch_br(key, plan_br_launch(key, count, a.acc_dbg != nullptr), a);
    hip_check(hipGetLastError(), "blind_rotate launch");
    std::vector<int32_t> ubuf((size_t)total * dp.u_stride);
    d2h(ubuf.data(), a.u_buf, ubuf.size(), "download u");
    if (acc_out) d2h(acc_out, a.acc_dbg, (size_t)count * 2 * dp.N, "download acc");
    sync_stream(name);
    const size_t uw = (size_t)dp.k * dp.N + 1;
    for (int c = 0; c < count; ++c) {
        const size_t nout = (size_t)((c + 1 < count ? rots[c + 1].u_index : total) - rots[c].u_index);
        unpad_rows(u_out + (size_t)c * out_rows * uw, &ubuf[(size_t)rots[c].u_index * dp.u_stride], nout, uw, (size_t)dp.u_stride);
    }
    stats.blind_rotates += (uint64_t)count;
}

// the raw key-switch entries: plan.count rows up, row c into row c of a private pool by `plan`, the rows down.  name: the
// entry, for error messages
void Engine::run_keyswitch_rows(const DeviceKeyImage *key, const KsLaunchPlan &plan, const Torus32 *u, Torus32 *out, const char *name) {
    const DevParams &dp = key->dp;
    const int count = plan.count;
    const std::vector<int32_t> padded = pad_rows(u, (size_t)count, (size_t)dp.k * dp.N + 1, (size_t)dp.u_stride);
    const int32_t *u_buf = scratch_upload(S_EXTRACT, padded.data(), padded.size(), "upload u");
    std::vector<KsDesc> ks(count);
    for (int c = 0; c < count; ++c) ks[c] = KsDesc{c, -1, 0, c};
    const KsDesc *dks = scratch_upload(S_KS, ks.data(), ks.size(), "upload ks");
    int32_t *dpool = scratch_as<int32_t>(S_RAW_POOL, (size_t)count * dp.ct_stride);
    (void)scratch(S_KS_PARTIAL, plan.partial_bytes);
    launch_ks(key, plan, u_buf, dks, dpool);
    hip_check(hipGetLastError(), (std::string(name) + " launch").c_str());
    std::vector<int32_t> res((size_t)count * dp.ct_stride);
    d2h(res.data(), dpool, res.size(), "download ks");
    sync_stream(name);
    unpad_rows(out, res.data(), (size_t)count, (size_t)dp.n + 1, (size_t)dp.ct_stride);
    stats.keyswitches += (uint64_t)count;
}

void Engine::run_keyswitch(const DeviceKeyImage *key, const Torus32 *u, int count, Torus32 *out) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();
    run_keyswitch_rows(key, plan_ks_launch(key, count, false), u, out, "keyswitch");
}

void Engine::run_keyswitch_matrix(const DeviceKeyImage *key, const Torus32 *u, int count, Torus32 *out) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();
    const DevParams &dp = key->dp;
    if (count <= 0) api_fail("keyswitch_matrix: no rows");
    if (!ks_matrix_shape_ok(dp.k * dp.N, dp.ks_t, dp.ks_basebit)) api_fail("keyswitch_matrix: the key's shape has no matrix form");
    if (!ensure_ks_planes(key)) api_fail("keyswitch_matrix: out of device memory for the byte-plane image of the key");
    run_keyswitch_rows(key, ks_matrix_plan(count), u, out, "keyswitch_matrix");
}

double Engine::run_wg_times(const DeviceKeyImage *key, int width, unsigned long long *wg_times) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();
    const DevParams &dp = key->dp;
    if (width <= 0 || !wg_times || dp.N != 1024) return -1.0;       // the stamps come from the 4-wave kernel only
    // a private "pool": `width` random input ciphertexts
    std::vector<int32_t> host((size_t)width * dp.ct_stride);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (auto &w : host) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; w = (int32_t)(x >> 16); }
    int32_t *pool = scratch_as<int32_t>(S_PROBE_POOL, (size_t)width * dp.ct_stride);
    hip_check(hipMemcpy(pool, host.data(), host.size() * 4, hipMemcpyHostToDevice), "probe pool");
    std::vector<RotDesc> rots(width);
    for (int i = 0; i < width; ++i) rots[i] = RotDesc{i, (i + 1) % width, 1, 1, -dp.mu, i};
    RotDesc *drots = scratch_as<RotDesc>(S_PROBE_ROTS, rots.size());
    hip_check(hipMemcpy(drots, rots.data(), rots.size() * sizeof(RotDesc), hipMemcpyHostToDevice), "probe rots");
    int32_t *ubuf = scratch_as<int32_t>(S_PROBE_EXTRACT, (size_t)(width + 1) * dp.u_stride);
    unsigned long long *dtimes = scratch_as<unsigned long long>(S_PROBE_TIMES, (size_t)4 * width);
    hipStream_t st;
    hip_check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "probe stream");
    hipEvent_t e0, e1;
    hip_check(hipEventCreate(&e0), "probe event");
    hip_check(hipEventCreate(&e1), "probe event");
    // launches back to back, the last one stamped and timed: what a level of a circuit sees
    // (TFHE_HIP_PROBE_WARM = "count:width" changes the unstamped launches before it, default one of the same width)
    int warm_count = 1, warm_width = width;
    if (const char *env = std::getenv("TFHE_HIP_PROBE_WARM")) std::sscanf(env, "%d:%d", &warm_count, &warm_width);
    warm_width = std::max(1, std::min(warm_width, width));
    BrLaunch a{pool, drots, warm_width, ubuf, nullptr, st};
    for (int w = 0; w < warm_count; ++w) launch_br(key, plan_br_launch(key, warm_width, false), a);
    // cleared first so that a launch which wrote no stamps is noticed instead of read as timings
    hip_check(hipMemsetAsync(dtimes, 0, (size_t)4 * width * 8, st), "clear stamps");
    wg_times_dbg_ = dtimes;
    hip_check(hipEventRecord(e0, st), "probe event record");
    a.count = width;
    launch_br(key, plan_br_launch(key, width, false), a);
    hip_check(hipEventRecord(e1, st), "probe event record");
    hip_check(hipStreamSynchronize(st), "probe stamps");
    wg_times_dbg_ = nullptr;
    float ems = 0.f;
    hip_check(hipEventElapsedTime(&ems, e0, e1), "probe event time");
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    hip_check(hipMemcpy(wg_times, dtimes, (size_t)4 * width * 8, hipMemcpyDeviceToHost), "probe stamps copy");
    hip_check(hipStreamDestroy(st), "probe stream destroy");
    for (int i = 0; i < width; ++i)
        if (wg_times[4 * i] == 0 || wg_times[4 * i + 1] == 0) return -1.0;      // a workgroup left no stamp
    return (double)ems;
}

void Engine::run_negacyclic(const DeviceKeyImage *key, const int32_t *ip, const Torus32 *tp, Torus32 *res, int count) {
    ENGINE_DEVICE_SCOPE();
    wait_flight();
    DevParams dp = key->dp;
    dp.br_variant = tunings.br_variant == 2 ? 2 : 0;            // 2: through the split transforms
    const size_t words = (size_t)count * dp.N;
    uint32_t scale[2];
    image_scale(dp.N, scale);
    const int32_t *dtp = scratch_upload(S_NEGA_TP, tp, words, "upload tp");
    const int32_t *dip = scratch_upload(S_NEGA_IP, ip, words, "upload ip");
    uint32_t *dimg = scratch_as<uint32_t>(S_NEGA_IMG, words * 2);
    int32_t *dres = scratch_as<int32_t>(S_NEGA_RES, words);
    launch_bk_transform(stream_, dp, dtp, dimg, key->tw.get(), count, 1, scale);
    launch_negacyclic(stream_, dp, key->tw.get(), dip, dimg, dres, count);
    hip_check(hipGetLastError(), "negacyclic launch");
    d2h(res, dres, words, "download res");
    sync_stream("negacyclic");
}

// ---- packing key switch (pack.hpp, pack.hip) ------------------------------------------------
DeviceBuf<uint32_t> Engine::upload_pack_image(const DeviceKeyImage *key, const Torus32 *rows, int t) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const ImageRows r{key->dp.n * t, 2, rows, nullptr, false,
                      {"the NTT image of a packing key", "the staging copy of a packing key", nullptr, "upload packing key", nullptr,
                       nullptr, "packing key transform", "packing key transform"}};
    return upload_image(key->dp, key->tw.get(), r, [](ImageStep) {});
}

DeviceBuf<uint32_t> Engine::expand_pack_image(const DeviceKeyImage *key, const uint32_t seed10[10], const Torus32 *body, int t) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const ImageRows r{key->dp.n * t, 2, body, seed10, true,
                      {"the NTT image of a packing key", "the staging copy of a packing key", "the bodies of a compressed packing key",
                       "upload packing key bodies", "packing key expand",
                       "packing key expand: arguments outside what the kernel was built for", "packing key transform",
                       "packing key expansion"}};
    DeviceBuf<uint32_t> img = upload_image(key->dp, key->tw.get(), r, [](ImageStep) {});
    ++seeded_stats.expanded_packing_keys;
    ++seeded_stats.packing_expand_launches;
    return img;
}

size_t Engine::read_pack_image(const DeviceBuf<uint32_t> &img, Torus32 *out, size_t capacity) {
    return read_back(img.bytes() / 4, out, capacity, "packing key image", [&] { return img.get(); });
}

void Engine::free_pack_image(DeviceBuf<uint32_t> &img) {
    free_image(!img.empty(), "sync before packing key free", [&] { img.reset(); });
}

void Engine::run_pack(const DeviceKeyImage *key, const uint32_t *img, int t, int basebit, SlotPool *pool, const int32_t *slots,
                      const Torus32 *raw_words, int count, int idx_per_wg, Torus32 *out, bool out_on_device, bool wait) {
    ENGINE_DEVICE_SCOPE();
    const DevParams &dp = key->dp;
    PackArgs a{};
    a.N = dp.N; a.n = dp.n; a.t = t; a.basebit = basebit; a.count = count;
    // one mask index per workgroup: n workgroups of two waves (630 at P128) over the chip's 1,024 SIMDs
    a.idx_per_wg = idx_per_wg > 0 ? idx_per_wg : 1;
    a.img = img; a.tw = key->tw.get();
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    const size_t out_words = (size_t)2 * dp.N, raw_words_n = (size_t)count * (dp.n + 1);
    a.partial = scratch_as<int32_t>(S_PACK_PARTIAL, (size_t)pack_groups(a.n, a.idx_per_wg) * out_words);
    int32_t *dslots = slots ? scratch_as<int32_t>(S_PACK_SLOTS, (size_t)count) : nullptr;
    int32_t *draw = slots ? nullptr : scratch_as<int32_t>(S_PACK_RAW, raw_words_n);
    a.out = out_on_device ? out : scratch_as<int32_t>(S_PACK_OUT, out_words);
    a.samples = slots ? pool->data() : draw;
    a.stride = slots ? pool->ct_stride() : dp.n + 1;
    a.slots = dslots;
    if (slots) h2d_staged(dslots, slots, (size_t)count, "upload slot list");
    else h2d(draw, raw_words, raw_words_n, "upload sample words");
    if (!launch_pack(stream_, a)) api_fail("pack: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "pack launch");
    if (!out_on_device) d2h(out, a.out, out_words, "download packed words");
    // (the raw form's upload reads the caller's pageable memory: it waits like a host destination)
    finish(wait || !out_on_device || !slots, "pack");
}

// ---- private selection (cmux.hpp, cmux.hip) --------------------------------------------------
static CmuxArgs cmux_args(const RingImage *sel, const Params &p) {
    CmuxArgs a{};
    a.N = p.N; a.l = p.l; a.Bgbit = p.Bgbit; a.offset = p.decomp_offset();
    a.img = sel->img.get(); a.tw = sel->tw.get();
    return a;
}

RingImage *Engine::upload_selector(const Params &p, const Torus32 *words, int nbits) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    auto sel = std::make_unique<RingImage>();
    sel->tw = upload_twiddles(p.N, "the twiddle tables of a selector");
    DevParams dp{};
    dp.N = p.N;
    const ImageRows r{nbits * p.kpl(), p.k + 1, words, nullptr, false,
                      {"the NTT image of a selector", "the staging copy of a selector", nullptr, "upload selector", nullptr,
                       nullptr, "selector transform", "selector transform"}};
    sel->img = upload_image(dp, sel->tw.get(), r, [](ImageStep) {});
    return sel.release();
}

RingImage *Engine::upload_selector_seeded(const Params &p, const uint32_t seed10[10], const Torus32 *bodies, int nbits) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    auto sel = std::make_unique<RingImage>();
    sel->tw = upload_twiddles(p.N, "the twiddle tables of a selector");
    DevParams dp{};
    dp.N = p.N;
    const ImageRows r{nbits * p.kpl(), p.k + 1, bodies, seed10, true,
                      {"the NTT image of a selector", "the staging copy of a selector", "the bodies of a compressed selector",
                       "upload selector bodies", "selector expand", "selector expand: arguments outside what the kernel was built for",
                       "selector transform", "selector expansion"}};
    sel->img = upload_image(dp, sel->tw.get(), r, [](ImageStep) {});
    return sel.release();
}

void Engine::free_selector(RingImage *sel) { free_image(sel, "sync before selector free", [&] { delete sel; }); }

// the event pair last_select_ms reads, made by the first timed launch
void Engine::ensure_select_events() {
    if (!kernel_timing || select_e0_) return;
    hip_check(hipEventCreate(&select_e0_), "select event");
    hip_check(hipEventCreate(&select_e1_), "select event");
}

void Engine::run_lookup(const RingImage *sel, const Params &p, int nbits, const Torus32 *ring, int M, int width, bool ring_on_device,
                        Torus32 *out, bool out_on_device) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)(p.k + 1) * p.N;
    // S = N / width entries rest in one sample: R samples, nbits - s tree levels over them, then s rotations
    int s = 0;
    while ((width << s) < p.N) ++s;
    const int R = (int)(((int64_t)M + (p.N / width) - 1) / (p.N / width)), levels = nbits - s;
    // every buffer first (scratch() may throw: nothing has been enqueued then).  Level j holds ceil(R / 2^(j+1)) entries:
    // the ping buffer is sized for level 0, the pong buffer for level 1; a rotation's one sample fits either
    int32_t *dring = ring_on_device ? nullptr : scratch_as<int32_t>(S_SELECT_RING, (size_t)R * sw);
    int32_t *lvl[2] = {nbits > 0 ? scratch_as<int32_t>(S_SELECT_A, (size_t)((R + 1) / 2) * sw) : nullptr,
                       nbits > 1 ? scratch_as<int32_t>(S_SELECT_B, (size_t)((R + 3) / 4) * sw) : nullptr};
    ensure_select_events();
    if (!ring_on_device) h2d_staged(dring, ring, (size_t)R * sw, "upload ring words");
    const int32_t *src = ring_on_device ? ring : dring;
    if (kernel_timing) hip_check(hipEventRecord(select_e0_, stream_), "select event");
    int cnt = R;
    for (int j = 0; j < nbits; ++j) {
        CmuxArgs a = cmux_args(sel, p);
        if (j < levels) {
            a.bit = s + j; a.count = (cnt + 1) / 2; a.n_d1 = cnt / 2;
            a.stride = (int64_t)2 * sw; a.d0 = src; a.d1 = src + sw;
        } else {
            // c <- ROT(G_t, width 2^t, c), t = j - levels: the one sample the tree left (cnt = 1)
            a.bit = j - levels; a.rot = width << (j - levels); a.count = 1; a.n_d1 = 0;
            a.stride = (int64_t)sw; a.d0 = src;
        }
        a.out = j == nbits - 1 && out_on_device ? out : lvl[j & 1];
        if (!launch_cmux(stream_, a)) api_fail("select: arguments outside what the CMUX kernel was built for");
        hip_check(hipGetLastError(), "cmux launch");
        src = a.out;
        cnt = a.count;
    }
    if (kernel_timing) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    select_timed_ = kernel_timing;
    if (!out_on_device) d2h(out, src, sw, "download selected words");
    else if (nbits == 0) hip_check(hipMemcpyAsync(out, src, sw * 4, hipMemcpyDeviceToDevice, stream_), "copy selected words");
    finish(!ring_on_device || !out_on_device, "select");
}

void Engine::run_cmux(const RingImage *sel, const Params &p, int bit, const Torus32 *d1, const Torus32 *d0, int count, Torus32 *out,
                      int rot) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t words = (size_t)count * (p.k + 1) * p.N;
    int32_t *dd0 = scratch_as<int32_t>(S_SELECT_RING, words), *dd1 = rot ? nullptr : scratch_as<int32_t>(S_CMUX_D1, words);
    int32_t *dout = scratch_as<int32_t>(S_SELECT_A, words);
    h2d(dd0, d0, words, "upload d0 words");
    if (!rot) h2d(dd1, d1, words, "upload d1 words");
    CmuxArgs a = cmux_args(sel, p);
    a.bit = bit; a.count = count; a.n_d1 = rot ? 0 : count; a.rot = rot;
    a.stride = (int64_t)(p.k + 1) * p.N; a.d0 = dd0; a.d1 = dd1; a.out = dout;
    if (!launch_cmux(stream_, a)) api_fail("cmux: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "cmux launch");
    d2h(out, dout, words, "download cmux words");
    finish(true, "cmux");
}

double Engine::last_select_ms() {
    ENGINE_DEVICE_SCOPE();
    if (!select_timed_) return -1.0;
    wait_event(select_e1_, "select event", sync_deadline_ms, diag_label);
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, select_e0_, select_e1_), "select event");
    return ms;
}

// ---- ring-encrypted inputs (unpack.hpp, unpack.hip) -----------------------------------------
// The tail run_unpack and run_inner share: `count` rows of u_stride words, made chunk by chunk, and their key switch.
// size_rows sizes every buffer of it (scratch() may throw: nothing has been enqueued then).  The key switches run by two
// plans, the widest chunk's and the last one's (which may be cut into more ranges); the partial sums are sized for both
Engine::RowsPlan Engine::size_rows(const DeviceKeyImage *key, int u_stride, int count, bool to_slots) {
    RowsPlan r;
    r.widest = std::min(count, UNPACK_CHUNK);
    r.u_stride = u_stride;
    r.dks = to_slots ? scratch_as<KsDesc>(S_UNPACK_KS, (size_t)count) : nullptr;
    r.u_buf = scratch_as<int32_t>(S_UNPACK_EXTRACT, (size_t)r.widest * u_stride);
    if (to_slots) {
        r.ks_wide = plan_ks_launch(key, r.widest, false);
        r.ks_last = plan_ks_launch(key, count - (count - 1) / UNPACK_CHUNK * UNPACK_CHUNK, false);
        (void)scratch(S_KS_PARTIAL, std::max(r.ks_wide.partial_bytes, r.ks_last.partial_bytes));
    }
    return r;
}

// make_rows(done, cnt): the launch that writes rows done .. done + cnt - 1 of the call into r.u_buf[0 .. cnt).  The slot
// form (u_out null): the key switch of row j goes into pool slot slots[j]; the raw form: the rows alone, [count][uw]
template <class MakeRows>
void Engine::run_rows(const DeviceKeyImage *key, const RowsPlan &r, int count, size_t uw, SlotPool *pool, const int32_t *slots,
                      Torus32 *u_out, const char *what, MakeRows &&make_rows) {
    if (!u_out) {
        std::vector<KsDesc> hks((size_t)count);
        for (int j = 0; j < count; ++j) hks[j] = KsDesc{j % UNPACK_CHUNK, -1, 0, slots[j]};
        h2d_staged(r.dks, hks.data(), hks.size(), "upload unpack ks");
    }
    std::vector<int32_t> rows(u_out ? (size_t)r.widest * r.u_stride : 0);
    for (int done = 0; done < count; done += UNPACK_CHUNK) {
        const int cnt = std::min(UNPACK_CHUNK, count - done);
        make_rows(done, cnt);
        last_extract_words_ = (size_t)cnt * r.u_stride;
        if (u_out) {
            d2h(rows.data(), r.u_buf, (size_t)cnt * r.u_stride, "download extracted rows");
            sync_stream(what);
            unpad_rows(u_out + (size_t)done * uw, rows.data(), (size_t)cnt, uw, (size_t)r.u_stride);
        } else {
            // (the next chunk's rows are ordered behind this key switch: one stream, one buffer)
            launch_ks(key, cnt == r.widest ? r.ks_wide : r.ks_last, r.u_buf, r.dks + done, pool->data());
            hip_check(hipGetLastError(), "unpack keyswitch launch");
        }
    }
    if (!u_out) stats.keyswitches += (uint64_t)count;
}

void Engine::run_unpack(const DeviceKeyImage *key, const Torus32 *ring_words, int nring, bool ring_on_device, const int32_t *index,
                        int count, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait, bool seeded) {
    ENGINE_DEVICE_SCOPE();
    const DevParams &dp = key->dp;
    const size_t ring_count = (size_t)nring * (seeded ? RING_SEED_WORDS + dp.N : 2 * dp.N), uw = (size_t)dp.k * dp.N + 1;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dring = ring_on_device ? nullptr : scratch_as<int32_t>(S_UNPACK_RING, ring_count);
    int32_t *dindex = scratch_as<int32_t>(S_UNPACK_INDEX, (size_t)count);
    const RowsPlan r = size_rows(key, dp.u_stride, count, !u_out);
    h2d_staged(dindex, index, (size_t)count, "upload unpack index");
    if (!ring_on_device) h2d(dring, ring_words, ring_count, "upload ring words");
    const int32_t *src = ring_on_device ? ring_words : dring;
    run_rows(key, r, count, uw, pool, slots, u_out, "ring extract", [&](int done, int cnt) {
        if (seeded ? !launch_ring_extract_seeded(stream_, UnpackSeededArgs{dp.N, cnt, dp.u_stride, src, dindex + done, r.u_buf})
                   : !launch_ring_extract(stream_, UnpackArgs{dp.N, cnt, dp.u_stride, src, dindex + done, r.u_buf}))
            api_fail("unpack: arguments outside what the extract kernel was built for");
        hip_check(hipGetLastError(), "ring extract launch");
        ++stats.unpack_launches;
        if (seeded) ++seeded_stats.seeded_unpack_launches;
    });
    if (u_out) return;
    stats.unpacked_samples += (uint64_t)count;
    if (seeded) seeded_stats.seeded_unpacked_samples += (uint64_t)count;
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(wait || !ring_on_device, "unpack");
}

// ---- encrypted inner products (cmux.hpp InnerArgs, cmux.hip inner_kernel) ---------------------
void Engine::run_inner(const RingImage *sel, const Params &p, int bit, const DeviceKeyImage *key, const Torus32 *ring, int R,
                       bool ring_on_device, int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, Torus32 *prod_out,
                       bool wait) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)(p.k + 1) * p.N;
    const int S = p.N / width;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dring = ring_on_device ? nullptr : scratch_as<int32_t>(S_SELECT_RING, (size_t)R * sw);
    InnerArgs x{cmux_args(sel, p), RingRows{}};
    x.c.bit = bit; x.c.stride = (int64_t)sw;
    if (prod_out) {
        // the raw product form: one launch over all R samples, no rows
        x.c.out = scratch_as<int32_t>(S_SELECT_A, (size_t)R * sw);
        h2d(dring, ring, (size_t)R * sw, "upload ring words");
        x.c.d0 = dring; x.c.count = R;
        if (!launch_inner(stream_, x)) api_fail("ring product: arguments outside what the kernel was built for");
        hip_check(hipGetLastError(), "ring product launch");
        d2h(prod_out, x.c.out, (size_t)R * sw, "download product words");
        finish(true, "ring product");
        return;
    }
    const RowsPlan r = size_rows(key, p.u_stride(), M, !u_out);
    ensure_select_events();
    if (!ring_on_device) h2d(dring, ring, (size_t)R * sw, "upload ring words");
    const int32_t *src = ring_on_device ? ring : dring;
    x.rows.width = width; x.rows.u_stride = r.u_stride; x.rows.u_buf = r.u_buf;
    run_rows(key, r, M, (size_t)p.k * p.N + 1, pool, slots, u_out, "ring inner", [&](int done, int cnt) {
        // a chunk starts on a sample: S divides UNPACK_CHUNK (both powers of two, S <= N <= UNPACK_CHUNK)
        x.c.d0 = src + (size_t)(done / S) * sw; x.c.count = (cnt + S - 1) / S; x.rows.M = cnt;
        if (kernel_timing && done == 0) hip_check(hipEventRecord(select_e0_, stream_), "select event");
        if (!launch_inner(stream_, x)) api_fail("ring inner: arguments outside what the kernel was built for");
        hip_check(hipGetLastError(), "ring inner launch");
        if (kernel_timing && done + cnt == M) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    });
    select_timed_ = kernel_timing;
    if (u_out) return;
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(wait || !ring_on_device, "ring inner");
}

// ---- sums of TGSW products over several ring samples (ring_inner_sum.hpp, ring_inner_sum.hip) ----
static InnerSumArgs inner_sum_args(const RingImage *sel, const Params &p, int bit, int terms) {
    InnerSumArgs x{cmux_args(sel, p), terms, inner_sum_block_rows(p.N), RingRows{}};
    x.c.bit = bit; x.c.stride = (int64_t)terms * (p.k + 1) * p.N;
    return x;
}

void Engine::run_inner_sum_mul(const RingImage *sel, const Params &p, int bit, int terms, const Torus32 *ring, int G, bool on_device,
                               Torus32 *out) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)(p.k + 1) * p.N;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dring = on_device ? nullptr : scratch_as<int32_t>(S_SELECT_RING, (size_t)G * terms * sw);
    int32_t *dout = on_device ? out : scratch_as<int32_t>(S_SELECT_A, (size_t)G * sw);
    ensure_select_events();
    if (!on_device) h2d(dring, ring, (size_t)G * terms * sw, "upload ring words");
    InnerSumArgs x = inner_sum_args(sel, p, bit, terms);
    x.c.d0 = on_device ? ring : dring; x.c.count = G; x.c.out = dout;
    if (kernel_timing) hip_check(hipEventRecord(select_e0_, stream_), "select event");
    if (!launch_inner_sum(stream_, x)) api_fail("ring mul tgsw sum: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "ring mul tgsw sum launch");
    if (kernel_timing) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    select_timed_ = kernel_timing;
    if (!on_device) d2h(out, dout, (size_t)G * sw, "download product words");
    finish(!on_device, "ring mul tgsw sum");
}

void Engine::run_inner_sum(const RingImage *sel, const Params &p, int bit, int terms, const DeviceKeyImage *key, const Torus32 *ring, int G,
                           bool ring_on_device, int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t gw = (size_t)terms * (p.k + 1) * p.N;
    const int S = p.N / width;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dring = ring_on_device ? nullptr : scratch_as<int32_t>(S_SELECT_RING, (size_t)G * gw);
    const RowsPlan r = size_rows(key, p.u_stride(), M, !u_out);
    ensure_select_events();
    if (!ring_on_device) h2d(dring, ring, (size_t)G * gw, "upload ring words");
    const int32_t *src = ring_on_device ? ring : dring;
    InnerSumArgs x = inner_sum_args(sel, p, bit, terms);
    x.rows.width = width; x.rows.u_stride = r.u_stride; x.rows.u_buf = r.u_buf;
    run_rows(key, r, M, (size_t)p.k * p.N + 1, pool, slots, u_out, "ring inner sum", [&](int done, int cnt) {
        // a chunk starts on a group: S divides UNPACK_CHUNK (both powers of two, S <= N <= UNPACK_CHUNK)
        x.c.d0 = src + (size_t)(done / S) * gw; x.c.count = (cnt + S - 1) / S; x.rows.M = cnt;
        if (kernel_timing && done == 0) hip_check(hipEventRecord(select_e0_, stream_), "select event");
        if (!launch_inner_sum(stream_, x)) api_fail("ring inner sum: arguments outside what the kernel was built for");
        hip_check(hipGetLastError(), "ring inner sum launch");
        if (kernel_timing && done + cnt == M) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    });
    select_timed_ = kernel_timing;
    if (u_out) return;
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(wait || !ring_on_device, "ring inner sum");
}

// ---- ring sample times public polynomials (ring_public.hpp, ring_public.hip) -----------------
RingImage *Engine::upload_public(int N, const int32_t *polys, int R) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t raw_words = (size_t)R * N;
    auto g = std::make_unique<RingImage>();
    g->tw = upload_twiddles(N, "the twiddle tables of a public gallery");
    g->img = DeviceBuf<uint32_t>(raw_words * 2, "the NTT image of a public gallery");
    DeviceBuf<int32_t> raw(raw_words, "the staging copy of a public gallery");
    hip_check(hipMemcpy(raw.get(), polys, raw_words * 4, hipMemcpyHostToDevice), "upload public gallery");
    PublicImageArgs a{};
    image_scale(N, a.scale);
    a.N = N; a.count = R; a.polys = raw.get(); a.img = g->img.get(); a.tw = g->tw.get();
    if (!launch_public_image(stream_, a)) fatal("public gallery transform: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "public gallery transform launch");
    sync_stream("public gallery transform");
    return g.release();
}

void Engine::free_public(RingImage *g) { free_image(g, "sync before public gallery free", [&] { delete g; }); }

void Engine::run_public_mul(const RingImage *g, int N, int first, int img_step, const Torus32 *ring, int nsamples, int total,
                            bool on_device, Torus32 *out) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)2 * N;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dring = on_device ? nullptr : scratch_as<int32_t>(S_PUBLIC_RING, (size_t)nsamples * sw);
    int32_t *dout = on_device ? out : scratch_as<int32_t>(S_PUBLIC_OUT, (size_t)total * sw);
    ensure_select_events();
    if (!on_device) h2d(dring, ring, (size_t)nsamples * sw, "upload ring words");
    PublicArgs a{};
    a.N = N; a.count = total; a.img_step = img_step; a.ring_stride = nsamples == 1 ? 0 : (int64_t)sw;
    a.ring = on_device ? ring : dring; a.img = g->img.get() + (size_t)first * sw; a.tw = g->tw.get(); a.out = dout;
    if (kernel_timing) hip_check(hipEventRecord(select_e0_, stream_), "select event");
    if (!launch_public(stream_, a)) api_fail("ring mul public: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "ring mul public launch");
    if (kernel_timing) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    select_timed_ = kernel_timing;
    if (!on_device) d2h(out, dout, (size_t)total * sw, "download product words");
    finish(!on_device, "ring mul public");
}

void Engine::run_public_inner(const RingImage *g, const Params &p, const DeviceKeyImage *key, const Torus32 *probe, bool probe_on_device,
                              int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out, bool wait) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)2 * p.N;
    const int S = p.N / width;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dprobe = probe_on_device ? nullptr : scratch_as<int32_t>(S_PUBLIC_RING, sw);
    const RowsPlan r = size_rows(key, p.u_stride(), M, !u_out);
    ensure_select_events();
    if (!probe_on_device) h2d(dprobe, probe, sw, "upload probe words");
    PublicArgs a{};
    a.N = p.N; a.img_step = 1; a.ring_stride = 0; a.ring = probe_on_device ? probe : dprobe; a.tw = g->tw.get();
    a.rows.width = width; a.rows.u_stride = r.u_stride; a.rows.u_buf = r.u_buf;
    run_rows(key, r, M, (size_t)p.k * p.N + 1, pool, slots, u_out, "ring inner public", [&](int done, int cnt) {
        // a chunk starts on a polynomial: S divides UNPACK_CHUNK (both powers of two, S <= N <= UNPACK_CHUNK)
        a.img = g->img.get() + (size_t)(done / S) * sw; a.count = (cnt + S - 1) / S; a.rows.M = cnt;
        if (kernel_timing && done == 0) hip_check(hipEventRecord(select_e0_, stream_), "select event");
        if (!launch_public(stream_, a)) api_fail("ring inner public: arguments outside what the kernel was built for");
        hip_check(hipGetLastError(), "ring inner public launch");
        if (kernel_timing && done + cnt == M) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    });
    select_timed_ = kernel_timing;
    if (u_out) return;
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(wait || !probe_on_device, "ring inner public");
}

void Engine::run_public_sum_mul(const RingImage *g, int N, int first, int terms, int ngroups, const Torus32 *ring, bool on_device,
                                Torus32 *out) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)2 * N;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dring = on_device ? nullptr : scratch_as<int32_t>(S_PUBLIC_RING, (size_t)terms * sw);
    int32_t *dout = on_device ? out : scratch_as<int32_t>(S_PUBLIC_OUT, (size_t)ngroups * sw);
    ensure_select_events();
    if (!on_device) h2d(dring, ring, (size_t)terms * sw, "upload ring words");
    PublicSumArgs a{};
    a.N = N; a.count = ngroups; a.terms = terms;
    a.ring = on_device ? ring : dring; a.img = g->img.get() + (size_t)first * sw; a.tw = g->tw.get(); a.out = dout;
    if (kernel_timing) hip_check(hipEventRecord(select_e0_, stream_), "select event");
    if (!launch_public_sum(stream_, a)) api_fail("ring mul public sum: arguments outside what the kernel was built for");
    hip_check(hipGetLastError(), "ring mul public sum launch");
    if (kernel_timing) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    select_timed_ = kernel_timing;
    if (!on_device) d2h(out, dout, (size_t)ngroups * sw, "download product words");
    finish(!on_device, "ring mul public sum");
}

void Engine::run_public_sum_inner(const RingImage *g, const Params &p, const DeviceKeyImage *key, int terms, const Torus32 *probe,
                                  bool probe_on_device, int M, int width, SlotPool *pool, const int32_t *slots, Torus32 *u_out,
                                  bool wait) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t sw = (size_t)2 * p.N;
    const int S = p.N / width;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *dprobe = probe_on_device ? nullptr : scratch_as<int32_t>(S_PUBLIC_RING, (size_t)terms * sw);
    const RowsPlan r = size_rows(key, p.u_stride(), M, !u_out);
    ensure_select_events();
    if (!probe_on_device) h2d(dprobe, probe, (size_t)terms * sw, "upload probe words");
    PublicSumArgs a{};
    a.N = p.N; a.terms = terms; a.ring = probe_on_device ? probe : dprobe; a.tw = g->tw.get();
    a.rows.width = width; a.rows.u_stride = r.u_stride; a.rows.u_buf = r.u_buf;
    run_rows(key, r, M, (size_t)p.k * p.N + 1, pool, slots, u_out, "ring inner public sum", [&](int done, int cnt) {
        // a chunk starts on a group: S divides UNPACK_CHUNK (both powers of two, S <= N <= UNPACK_CHUNK)
        a.img = g->img.get() + (size_t)(done / S) * terms * sw; a.count = (cnt + S - 1) / S; a.rows.M = cnt;
        if (kernel_timing && done == 0) hip_check(hipEventRecord(select_e0_, stream_), "select event");
        if (!launch_public_sum(stream_, a)) api_fail("ring inner public sum: arguments outside what the kernel was built for");
        hip_check(hipGetLastError(), "ring inner public sum launch");
        if (kernel_timing && done + cnt == M) hip_check(hipEventRecord(select_e1_, stream_), "select event");
    });
    select_timed_ = kernel_timing;
    if (u_out) return;
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(wait || !probe_on_device, "ring inner public sum");
}

// ---- ring LUT bootstrap (ring_rotate.hpp, ring_rotate.hip) -------------------------------------
// every operand buffer of `count` rotations (scratch() may throw: nothing has been enqueued then), and the launch
// arguments that do not change from chunk to chunk
Engine::RotateOperands Engine::size_ring_rotate(const DeviceKeyImage *key, int nring, bool ring_on_device, const int32_t *ring_index,
                                                SlotPool *pool, int count) {
    const DevParams &dp = key->dp;
    RotateOperands o{};
    o.dring = ring_on_device ? nullptr : scratch_as<int32_t>(S_ROTATE_RING, (size_t)nring * 2 * dp.N);
    o.dindex = ring_index ? scratch_as<int32_t>(S_ROTATE_INDEX, (size_t)count) : nullptr;
    o.dslots = pool ? scratch_as<int32_t>(S_ROTATE_SLOTS, (size_t)count) : nullptr;
    o.dlwe = pool ? nullptr : scratch_as<int32_t>(S_ROTATE_LWE, (size_t)count * (dp.n + 1));
    RingRotateArgs &a = o.a;
    a.N = dp.N; a.l = dp.l; a.Bgbit = dp.Bgbit; a.n = dp.n; a.offset = dp.decomp_offset;
    // the cloud key's bootstrapping image and twiddle tables as they rest: nothing is uploaded again
    a.img = key->bk_img.get(); a.tw = key->tw.get();
    a.lwe = pool ? pool->data() : o.dlwe;
    a.lwe_stride = pool ? pool->ct_stride() : dp.n + 1;
    if (kernel_timing && !rotate_e0_) {
        hip_check(hipEventCreate(&rotate_e0_), "ring rotate event");
        hip_check(hipEventCreate(&rotate_e1_), "ring rotate event");
    }
    return o;
}

void Engine::upload_ring_rotate(RotateOperands &o, const DeviceKeyImage *key, const Torus32 *ring, int nring, bool ring_on_device,
                                const int32_t *ring_index, SlotPool *pool, const int32_t *in_slots, const Torus32 *lwe_words, int count) {
    const DevParams &dp = key->dp;
    if (ring_index) h2d_staged(o.dindex, ring_index, (size_t)count, "upload ring index");
    if (pool) h2d_staged(o.dslots, in_slots, (size_t)count, "upload slot list");
    else h2d(o.dlwe, lwe_words, (size_t)count * (dp.n + 1), "upload sample words");
    if (!ring_on_device) h2d(o.dring, ring, (size_t)nring * 2 * dp.N, "upload ring words");
    o.a.ring = ring_on_device ? ring : o.dring;
}

void Engine::run_ring_rotate(const DeviceKeyImage *key, const Torus32 *ring, int nring, bool ring_on_device, const int32_t *ring_index,
                             SlotPool *pool, const int32_t *in_slots, const Torus32 *lwe_words, int count, Torus32 *out,
                             bool out_on_device) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const size_t out_words = (size_t)count * 2 * key->dp.N;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    RotateOperands o = size_ring_rotate(key, nring, ring_on_device, ring_index, pool, count);
    int32_t *dout = out_on_device ? out : scratch_as<int32_t>(S_ROTATE_OUT, out_words);
    upload_ring_rotate(o, key, ring, nring, ring_on_device, ring_index, pool, in_slots, lwe_words, count);
    o.a.ring_index = o.dindex; o.a.lwe_index = o.dslots; o.a.count = count; o.a.out = dout;
    if (kernel_timing) hip_check(hipEventRecord(rotate_e0_, stream_), "ring rotate event");
    if (!launch_ring_rotate(stream_, o.a)) api_fail(std::string("ring rotate: ") + ring_rotate_error(o.a));
    hip_check(hipGetLastError(), "ring rotate launch");
    if (kernel_timing) hip_check(hipEventRecord(rotate_e1_, stream_), "ring rotate event");
    rotate_timed_ = kernel_timing;
    if (!out_on_device) d2h(out, dout, out_words, "download rotated words");
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(!ring_on_device || !out_on_device || !pool, "ring rotate");
}

void Engine::run_ring_rotate_rows(const DeviceKeyImage *key, const Torus32 *ring, int nring, bool ring_on_device, const int32_t *ring_index,
                                  SlotPool *pool, const int32_t *in_slots, const Torus32 *lwe_words, int count, const int32_t *out_slots,
                                  Torus32 *u_out, bool wait) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const DevParams &dp = key->dp;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    RotateOperands o = size_ring_rotate(key, nring, ring_on_device, ring_index, pool, count);
    const RowsPlan r = size_rows(key, dp.u_stride, count, !u_out);
    upload_ring_rotate(o, key, ring, nring, ring_on_device, ring_index, pool, in_slots, lwe_words, count);
    o.a.rows.width = dp.N; o.a.rows.u_stride = r.u_stride; o.a.rows.u_buf = r.u_buf;
    // (the slot form's results go to the caller's pool, which is the LWE samples' own when they rest in slots)
    run_rows(key, r, count, (size_t)dp.k * dp.N + 1, pool, out_slots, u_out, "ring rotate rows", [&](int done, int cnt) {
        o.a.ring_index = o.dindex ? o.dindex + done : nullptr;
        o.a.lwe_index = o.dslots ? o.dslots + done : nullptr;
        // without a list rotation j takes sample j: a chunk starts `done` samples on
        if (!o.dindex) o.a.ring = (ring_on_device ? ring : o.dring) + (size_t)done * 2 * dp.N;
        if (!o.dslots) o.a.lwe = o.dlwe + (size_t)done * (dp.n + 1);
        o.a.count = cnt; o.a.rows.M = cnt;
        if (kernel_timing && done == 0) hip_check(hipEventRecord(rotate_e0_, stream_), "ring rotate event");
        if (!launch_ring_rotate(stream_, o.a)) api_fail(std::string("ring rotate rows: ") + ring_rotate_error(o.a));
        hip_check(hipGetLastError(), "ring rotate launch");
        if (kernel_timing && done + cnt == count) hip_check(hipEventRecord(rotate_e1_, stream_), "ring rotate event");
    });
    rotate_timed_ = kernel_timing;
    if (u_out) return;
    // (a host source is the caller's pageable memory: its upload is waited for like a host destination)
    finish(wait || !ring_on_device, "ring rotate rows");
}

double Engine::last_ring_rotate_ms() {
    ENGINE_DEVICE_SCOPE();
    if (!rotate_timed_) return -1.0;
    wait_event(rotate_e1_, "ring rotate event", sync_deadline_ms, diag_label);
    float ms = 0.f;
    hip_check(hipEventElapsedTime(&ms, rotate_e0_, rotate_e1_), "ring rotate event");
    return ms;
}

size_t Engine::read_extract_rows(Torus32 *out, size_t capacity) {
    const size_t words = last_extract_words_;                     // (the buffer was sized by that launch: no growth)
    return read_back(words, out, capacity, "extract rows", [&] { return scratch_as<int32_t>(S_UNPACK_EXTRACT, words); });
}

// ---- seed-compressed LWE sample arrays (expand.hpp, expand.hip) ------------------------------
void Engine::run_lwe_expand(int n, int stride, const Torus32 *record, bool record_on_device, const int32_t *index, int count,
                            SlotPool *pool, const int32_t *slots, Torus32 *rows_out, bool wait) {
    ENGINE_DEVICE_SCOPE();
    ensure_init();
    const int widest = std::min(count, LWE_EXPAND_CHUNK);
    // the seed in front of the gathered bodies, padded so that they start on a 16-byte boundary
    constexpr size_t HEAD = (LWE_SEED_WORDS + 3) & ~(size_t)3;
    // every buffer first (scratch() may throw: nothing has been enqueued then)
    int32_t *drecord = record_on_device ? nullptr : scratch_as<int32_t>(S_LWE_RECORD, HEAD + (size_t)count);
    int32_t *dindex = scratch_as<int32_t>(S_LWE_INDEX, (size_t)count);
    int32_t *dslots = slots ? scratch_as<int32_t>(S_LWE_SLOTS, (size_t)count) : nullptr;
    int32_t *drows = slots ? pool->data() : scratch_as<int32_t>(S_LWE_ROWS, (size_t)widest * stride);
    h2d_staged(dindex, index, (size_t)count, "upload expand index");
    if (slots) h2d_staged(dslots, slots, (size_t)count, "upload slot list");
    if (!record_on_device) {
        std::vector<int32_t> up(HEAD + (size_t)count, 0);
        std::copy(record, record + LWE_SEED_WORDS, up.begin());
        for (int j = 0; j < count; ++j) up[HEAD + (size_t)j] = record[LWE_SEED_WORDS + (size_t)index[j]];
        h2d_staged(drecord, up.data(), up.size(), "upload seed and bodies");
    }
    const int32_t *seed = record_on_device ? record : drecord;
    std::vector<int32_t> rows(rows_out ? (size_t)widest * stride : 0);
    for (int done = 0; done < count; done += LWE_EXPAND_CHUNK) {
        const int cnt = std::min(LWE_EXPAND_CHUNK, count - done);
        LweExpandArgs a{};
        a.n = n; a.count = cnt; a.stride = stride; a.gathered = record_on_device ? 0 : 1;
        a.seed = reinterpret_cast<const uint32_t *>(seed);
        a.body = record_on_device ? record + LWE_SEED_WORDS : drecord + HEAD + done;
        a.index = dindex + done;
        a.slots = slots ? dslots + done : nullptr;
        a.rows = drows;
        if (!launch_lwe_expand(stream_, a)) api_fail("seeded import: arguments outside what the expand kernel was built for");
        hip_check(hipGetLastError(), "lwe expand launch");
        ++seeded_lwe_stats.seeded_import_launches;
        if (rows_out) {
            last_expand_words_ = (size_t)cnt * stride;
            d2h(rows.data(), drows, (size_t)cnt * stride, "download expanded rows");
            sync_stream("lwe expand");
            unpad_rows(rows_out + (size_t)done * (n + 1), rows.data(), (size_t)cnt, (size_t)n + 1, (size_t)stride);
        }
    }
    if (rows_out) return;
    seeded_lwe_stats.seeded_imported_samples += (uint64_t)count;
    finish(wait, "seeded import");
}

size_t Engine::read_expand_slots(Torus32 *out, size_t capacity) {
    const size_t words = last_expand_words_;                      // (the buffer was sized by that launch: no growth)
    return read_back(words, out, capacity, "expand slots", [&] { return scratch_as<int32_t>(S_LWE_ROWS, words); });
}

}  // namespace tfhe_hip
