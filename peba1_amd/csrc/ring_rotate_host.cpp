// ring_rotate_host.cpp -- host side of the ring LUT bootstrap (include/tfhe_hip.h "ring LUT bootstrap"): the C ABI of the
// blind rotation of an encrypted ring sample by LWE samples of the pool, of the rotation with extraction and key switch,
// and of the raw launch.  No arithmetic happens here (ring_rotate.hip); the admission test is cmux.hpp's
// (ring_rotate.hpp says why).  An object of its own in build.sh: shim.cpp's list of included files is closed
// (tests/test_host_sources_cpu.py).
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

namespace {

constexpr RunMessages ROTATE_INDEX{"the index samples belong to a parameter set of LWE dimension ", ", the cloud key to one of ",
                                   "count runs past the end of the index samples' array",
                                   "the index samples live in the pool of another ciphertext shape"};

// what every entry checks alike, in the order the header lists the refusals: the count, the ring index, the ring
const Params &rotation_checked(const std::string &w, const TFheGateBootstrappingCloudKeySet *bk, int32_t nring, const int32_t *ring_index,
                               int32_t count) {
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    if (count < 1 || count > ROTATE_MAX_COUNT) api_fail(w + "count must be in 1.." + std::to_string(ROTATE_MAX_COUNT));
    if (nring < 1) api_fail(w + "nring must be at least 1");
    if (!ring_index && count > nring) api_fail(w + "count runs past the last of the ring samples");
    for (int32_t j = 0; ring_index && j < count; ++j)
        if (ring_index[j] < 0 || ring_index[j] >= nring)
            api_fail(w + "ring_index " + std::to_string(ring_index[j]) + " at " + std::to_string(j) + " is outside 0.." + std::to_string(nring - 1));
    const Params &p = bk->bk->p;
    if (const char *why = cmux_gadget_error(p.N, p.k, p.l, p.Bgbit)) api_fail(w + why);
    return p;
}

// the index samples' current slots.  What is recorded runs first if one of them is the result of a recorded operation
// that has not run (sync_sample_locked's test, recorder.cpp) -- the slots are taken AFTER that flush, as pack_impl takes
// them --, and stays recorded otherwise
std::vector<int32_t> operand_slots(const LweSample *samples, int32_t count, SlotPool *pool) {
    bool pending = false;
    for (int32_t j = 0; j < count && !pending; ++j) {
        const int32_t s = samples[j].slot;                    // below 0: the value lives in the host mirror
        pending = s >= 0 && pool_of_sample(&samples[j]) == pool && pool->pending[s];
    }
    if (pending) flush_pending_locked(true);
    std::vector<int32_t> slots((size_t)count);
    for (int32_t j = 0; j < count; ++j) slots[(size_t)j] = ensure_slot(&samples[j], pool);
    return slots;
}

int rotate_impl(const char *who, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring, int32_t nring, const int32_t *ring_index,
                const LweSample *samples, int32_t count, Torus32 *out, bool on_device) {
    const std::string w = std::string(who) + ": ";
    const Params &p = rotation_checked(w, bk, nring, ring_index, count);
    if (!ring || !samples || !out) api_fail(w + "null ring words, index samples or destination");
    if (on_device) {
        const uintptr_t rb = reinterpret_cast<uintptr_t>(ring), ob = reinterpret_cast<uintptr_t>(out);
        if ((rb | ob) & 15) api_fail(w + "device words must be 16-byte aligned");
        const uintptr_t sb = (uintptr_t)(p.k + 1) * p.N * 4;
        if (rb < ob + (uintptr_t)count * sb && ob < rb + (uintptr_t)nring * sb) api_fail(w + "the destination overlaps the ring words");
    }
    auto g = recorder_lock();
    check_runs(w, ROTATE_INDEX, [&](int32_t) { return samples; }, 1, count, p);
    SlotPool *pool = pool_of_key(bk);
    const std::vector<int32_t> slots = operand_slots(samples, count, pool);
    // names no pool slot of its own; a flush in flight goes on (the launch is ordered behind it on the stream)
    Engine::get().run_ring_rotate(bk->bk->dev, ring, nring, on_device, ring_index, pool, slots.data(), nullptr, count, out, on_device);
    return 0;
}

int lut_impl(const char *who, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring, int32_t nring, const int32_t *ring_index,
             const LweSample *in, int32_t count, LweSample *out, bool on_device) {
    const std::string w = std::string(who) + ": ";
    const Params &p = rotation_checked(w, bk, nring, ring_index, count);
    if (!ring || !in || !out) api_fail(w + "null ring words, input samples or result");
    if (on_device && (reinterpret_cast<uintptr_t>(ring) & 15)) api_fail(w + "device words must be 16-byte aligned");
    auto g = recorder_lock();
    check_runs(w, ROTATE_INDEX, [&](int32_t) { return in; }, 1, count, p);
    // as the unpack: every result ours, of the key's LWE dimension, not bound to the pool of another shape
    check_runs(w, UNPACK_RESULT, ResultsView(out), count, p);
    SlotPool *pool = pool_of_key(bk);
    const std::vector<int32_t> slots = operand_slots(in, count, pool);
    // a flush in flight owns the key switch's partial sums; what is recorded and not involved stays recorded
    finish_flight_locked();
    import_into_fresh_slots(pool, ResultsView(out), count, [&](const int32_t *fresh) {
        Engine::get().run_ring_rotate_rows(bk->bk->dev, ring, nring, on_device, ring_index, pool, slots.data(), nullptr, count, fresh, nullptr,
                                           !on_device);
    });
    return 0;
}

}  // namespace

extern "C" {

int tfhe_hip_ring_blind_rotate(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_in, int32_t nring, const int32_t *ring_index,
                               const LweSample *index_samples, int32_t count, Torus32 *ring_out) {
    return guarded_rc([&] { return rotate_impl("tfhe_hip_ring_blind_rotate", bk, ring_in, nring, ring_index, index_samples, count, ring_out, false); });
}
int tfhe_hip_ring_blind_rotate_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_in, int32_t nring,
                                      const int32_t *ring_index, const LweSample *index_samples, int32_t count, void *device_ring_out) {
    return guarded_rc([&] {
        return rotate_impl("tfhe_hip_ring_blind_rotate_device", bk, static_cast<const Torus32 *>(device_ring_in), nring, ring_index, index_samples,
                           count, static_cast<Torus32 *>(device_ring_out), true);
    });
}

int tfhe_hip_ring_lut_bootstrap(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_tables, int32_t ntables,
                                const int32_t *ring_index, const LweSample *in, int32_t count, LweSample *out) {
    return guarded_rc([&] { return lut_impl("tfhe_hip_ring_lut_bootstrap", bk, ring_tables, ntables, ring_index, in, count, out, false); });
}
int tfhe_hip_ring_lut_bootstrap_device(const TFheGateBootstrappingCloudKeySet *bk, const void *device_ring_tables, int32_t ntables,
                                       const int32_t *ring_index, const LweSample *in, int32_t count, LweSample *out) {
    return guarded_rc([&] {
        return lut_impl("tfhe_hip_ring_lut_bootstrap_device", bk, static_cast<const Torus32 *>(device_ring_tables), ntables, ring_index, in, count,
                        out, true);
    });
}

int tfhe_hip_kernel_ring_rotate(const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *ring_words, int32_t nring, const int32_t *ring_index,
                                const Torus32 *lwe_words, int32_t count, Torus32 *out_ring_words, Torus32 *out_rows) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_ring_rotate: ";
        rotation_checked(w, bk, nring, ring_index, count);
        if (!ring_words || !lwe_words || (!out_ring_words && !out_rows)) api_fail(w + "null argument");
        auto g = recorder_lock();
        pool_of_key(bk);
        finish_flight_locked();                                   // (the row buffer is the unpack's)
        Engine &e = Engine::get();
        if (out_ring_words) e.run_ring_rotate(bk->bk->dev, ring_words, nring, false, ring_index, nullptr, nullptr, lwe_words, count, out_ring_words, false);
        if (out_rows)
            e.run_ring_rotate_rows(bk->bk->dev, ring_words, nring, false, ring_index, nullptr, nullptr, lwe_words, count, nullptr, out_rows, true);
        return 0;
    });
}

double tfhe_hip_last_ring_rotate_ms(void) {
    auto g = recorder_lock();
    return Engine::get().last_ring_rotate_ms();
}

}  // extern "C"
