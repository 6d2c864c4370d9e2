// inner_sum_host.cpp -- host side of the sums of TGSW products over several ring samples (include/tfhe_hip.h "TGSW products
// over several ring samples"): the C ABI of the summed product and of the summed inner products against an encrypted
// gallery.  No arithmetic happens here (ring_inner_sum.hip); the bounds a term count is checked against are
// ring_inner_sum.hpp's; the selector is select_host.cpp's.  An object of its own in build.sh: shim.cpp's list of included
// files is closed (tests/test_host_sources_cpu.py).
#include <string>

#include "shim_internal.hpp"

using namespace tfhe_hip;

static_assert(TFHE_HIP_INNER_MAX_TERMS == INNER_SUM_MAX_TERMS, "the header's cap is ring_inner_sum.hpp's");

namespace {

// the selector, its samples sample .. sample + terms - 1 and the term count its gadget admits: what every entry checks alike
void terms_checked(const std::string &w, const TfheHipSelector *sel, int32_t sample, int32_t terms) {
    selector_checked(w, sel);
    const int most = inner_sum_max_terms(sel->p.N, sel->p.l, sel->p.Bgbit);
    if (terms < 1 || terms > most)
        api_fail(w + "terms must be in 1.." + std::to_string(most) + " for this gadget (ring_inner_sum.hpp: the CRT bound, capped at " +
                 std::to_string(INNER_SUM_MAX_TERMS) + ")");
    if (sample < 0 || (int64_t)sample + terms > sel->nbits)
        api_fail(w + "sample_index .. sample_index + terms - 1 must lie in 0.." + std::to_string(sel->nbits - 1));
}

int mul_impl(const char *who, const TfheHipSelector *sel, int32_t sample, int32_t terms, int32_t ngroups, const Torus32 *ring, Torus32 *out,
             bool on_device, bool raw) {
    const std::string w = std::string(who) + ": ";
    if (!ring || !out) api_fail(w + "null ring words or destination");
    terms_checked(w, sel, sample, terms);
    if (ngroups < 1 || ngroups > INNER_SUM_MAX_GROUPS) api_fail(w + "ngroups must be in 1.." + std::to_string(INNER_SUM_MAX_GROUPS));
    if (on_device) {
        const uintptr_t rb = reinterpret_cast<uintptr_t>(ring), ob = reinterpret_cast<uintptr_t>(out);
        if ((rb | ob) & 15) api_fail(w + "device words must be 16-byte aligned");
        const uintptr_t sb = (uintptr_t)(sel->p.k + 1) * sel->p.N * 4;
        if (rb < ob + (uintptr_t)ngroups * sb && ob < rb + (uintptr_t)ngroups * terms * sb) api_fail(w + "the destination overlaps the ring words");
    }
    auto g = recorder_lock();
    if (raw) finish_flight_locked();
    // names no pool slot: what is recorded stays recorded, a flush in flight goes on (the launch is ordered behind it)
    const RingImage *img = select_image(sel);     // out of device memory: ApiError, nothing has changed
    Engine::get().run_inner_sum_mul(img, sel->p, sample, terms, ring, ngroups, on_device, out);
    return 0;
}

// every argument before the device is looked at, in the order the header lists the refusals
int inner_impl(const char *who, const TfheHipSelector *sel, int32_t sample, int32_t terms, const TFheGateBootstrappingCloudKeySet *bk,
               const Torus32 *ring, int32_t M, int32_t width, LweSample *result, bool on_device) {
    const std::string w = std::string(who) + ": ";
    if (!ring || !result) api_fail(w + "null ring words or result");
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    terms_checked(w, sel, sample, terms);
    const Params &p = bk->bk->p;
    const int N = sel->p.N;
    if (p.N != N || p.k != sel->p.k) api_fail(w + "the selector and the cloud key belong to different rings");
    if (width < 1 || width > N || (width & (width - 1))) api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
    if (M < 1) api_fail(w + "M must be at least 1");
    if (on_device && (reinterpret_cast<uintptr_t>(ring) & 15)) api_fail(w + "device words must be 16-byte aligned");
    const int S = N / width, G = (int)(((int64_t)M + S - 1) / S);
    auto g = recorder_lock();
    // as the unpack: every result ours, of the key's LWE dimension, not bound to the pool of another shape
    check_runs(w, UNPACK_RESULT, ResultsView(result), M, p);
    SlotPool *pool = pool_of_key(bk);
    // a flush in flight owns the key switch's partial sums; what is recorded and has not run stays recorded
    finish_flight_locked();
    const RingImage *img = select_image(sel);     // out of device memory: ApiError, nothing has changed
    import_into_fresh_slots(pool, ResultsView(result), M, [&](const int32_t *slots) {
        Engine::get().run_inner_sum(img, sel->p, sample, terms, bk->bk->dev, ring, G, on_device, M, width, pool, slots, nullptr, !on_device);
    });
    return 0;
}

}  // namespace

extern "C" {

int32_t tfhe_hip_ring_inner_sum_max_terms(const TFheGateBootstrappingParameterSet *params) {
    const std::string w = "tfhe_hip_ring_inner_sum_max_terms: ";
    if (!params || !params->in_out_params) { set_error(w + "null parameter set"); return -1; }
    const Params &p = params_of(params);
    if (const char *why = cmux_gadget_error(p.N, p.k, p.l, p.Bgbit)) { set_error(w + why); return -1; }
    return inner_sum_max_terms(p.N, p.l, p.Bgbit);
}

int tfhe_hip_ring_mul_tgsw_sum(const TfheHipSelector *sel, int32_t sample_index, int32_t terms, int32_t ngroups, const Torus32 *ring_words,
                               Torus32 *out_ring_words) {
    return guarded_rc([&] { return mul_impl("tfhe_hip_ring_mul_tgsw_sum", sel, sample_index, terms, ngroups, ring_words, out_ring_words, false, false); });
}
int tfhe_hip_ring_mul_tgsw_sum_device(const TfheHipSelector *sel, int32_t sample_index, int32_t terms, int32_t ngroups,
                                      const void *device_ring_words, void *device_out) {
    return guarded_rc([&] {
        return mul_impl("tfhe_hip_ring_mul_tgsw_sum_device", sel, sample_index, terms, ngroups, static_cast<const Torus32 *>(device_ring_words),
                        static_cast<Torus32 *>(device_out), true, false);
    });
}

int tfhe_hip_ring_inner_sum(const TfheHipSelector *sel, int32_t sample_index, int32_t terms, const TFheGateBootstrappingCloudKeySet *bk,
                            const Torus32 *ring_words, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] { return inner_impl("tfhe_hip_ring_inner_sum", sel, sample_index, terms, bk, ring_words, M, width, result, false); });
}
int tfhe_hip_ring_inner_sum_device(const TfheHipSelector *sel, int32_t sample_index, int32_t terms, const TFheGateBootstrappingCloudKeySet *bk,
                                   const void *device_ring_words, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] {
        return inner_impl("tfhe_hip_ring_inner_sum_device", sel, sample_index, terms, bk, static_cast<const Torus32 *>(device_ring_words), M, width,
                          result, true);
    });
}

int tfhe_hip_kernel_ring_inner_sum_product(const TfheHipSelector *sel, int32_t sample_index, int32_t terms, int32_t ngroups,
                                           const Torus32 *ring_words, Torus32 *out_words) {
    return guarded_rc(
        [&] { return mul_impl("tfhe_hip_kernel_ring_inner_sum_product", sel, sample_index, terms, ngroups, ring_words, out_words, false, true); });
}

int tfhe_hip_kernel_ring_inner_sum_rows(const TfheHipSelector *sel, int32_t sample_index, int32_t terms, const Torus32 *ring_words, int32_t G,
                                        int32_t M, int32_t width, Torus32 *out_rows) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_ring_inner_sum_rows: ";
        if (!ring_words || !out_rows) api_fail(w + "null argument");
        terms_checked(w, sel, sample_index, terms);
        if (G < 1 || G > INNER_SUM_MAX_GROUPS) api_fail(w + "G must be in 1.." + std::to_string(INNER_SUM_MAX_GROUPS));
        const int N = sel->p.N;
        if (width < 1 || width > N || (width & (width - 1))) api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
        const int64_t S = N / width;
        if (M <= (G - 1) * S || M > G * S) api_fail(w + "M must name an entry of the last of the G groups");
        auto g = recorder_lock();
        finish_flight_locked();                                   // (the row buffer is the unpack's)
        const RingImage *img = select_image(sel);
        Engine::get().run_inner_sum(img, sel->p, sample_index, terms, nullptr, ring_words, G, false, M, width, nullptr, nullptr, out_rows, true);
        return 0;
    });
}

int tfhe_hip_test_inner_sum_bounds(int32_t N, int32_t l, int32_t Bgbit, int32_t terms) {
    if ((N != 1024 && N != 2048) || l < 1 || Bgbit < 1 || Bgbit > CMUX_MAX_BGBIT || l * Bgbit > 32 || terms < 1 || terms > INNER_SUM_MAX_TERMS) {
        set_error("test_inner_sum_bounds: bad arguments");
        return -1;
    }
    // the MAC side: the block the kernel folds after -- the whole sum where it is shorter, with no fold under it then
    const int rows = terms * 2 * l, B = inner_sum_block_rows(N);
    const bool mac = rows <= B ? cmux_mac_ok(N, rows) : inner_sum_block_ok(N, B);
    return (mac ? 0 : 1) | (inner_sum_crt_ok(N, l, Bgbit, terms) ? 0 : 2);
}

int32_t tfhe_hip_test_inner_sum_block_rows(int32_t N) {
    if (N != 1024 && N != 2048) {
        set_error("test_inner_sum_block_rows: bad arguments");
        return -1;
    }
    return inner_sum_block_rows(N);
}

}  // extern "C"
