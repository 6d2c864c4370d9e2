// public_host.cpp -- host side of the products of ring samples with public polynomials (include/tfhe_hip.h "ring sample times
// public polynomials"): the gallery object and the C ABI of the product and of the inner products against a clear gallery.
// No arithmetic happens here (ring_public.hip); the bounds a gallery is checked against are ring_public.hpp's.  An object
// of its own in build.sh: shim.cpp's list of included files is closed (tests/test_host_sources_cpu.py).
#include <algorithm>
#include <string>
#include <vector>

#include "shim_internal.hpp"

using namespace tfhe_hip;

static_assert(TFHE_HIP_PUBLIC_MAX_COEF(1024) == public_max_coef(1024) && TFHE_HIP_PUBLIC_MAX_COEF(2048) == public_max_coef(2048),
              "the header's T is the one ring_public.hpp derives");
static_assert(TFHE_HIP_PUBLIC_MAX_TERMS == PUBLIC_MAX_TERMS && TFHE_HIP_PUBLIC_MAX_TERMS <= public_sum_mac_terms(1024) &&
                  TFHE_HIP_PUBLIC_MAX_TERMS <= public_sum_mac_terms(2048) && 2 * TFHE_HIP_PUBLIC_MAX_TERMS > public_sum_mac_terms(2048),
              "the header's term count is the largest power of two under the MAC bound ring_public.hpp derives (13 at N = 2048)");

// R polynomials [R][N] of a ring (N, k = 1); the device image is made at the first product (a gallery can be built and
// deleted on a machine without a GPU)
struct TfheHipPublicGallery {
    uint32_t magic;
    Params p;
    int32_t R;
    std::vector<int32_t> polys;
    RingImage *img;
    std::vector<int32_t> maxabs;     // max|q| of every polynomial, from construction (the CRT bound of a group of terms)
};

namespace {
constexpr uint32_t PUBLIC_MAGIC = 0x5055424Cu;

const TfheHipPublicGallery *gallery_checked(const std::string &w, const TfheHipPublicGallery *g) {
    if (!g || g->magic != PUBLIC_MAGIC) api_fail(w + "null or deleted gallery");
    return g;
}

// the gallery's image, made at first use (under the recorder lock)
const RingImage *gallery_image(const TfheHipPublicGallery *cg) {
    auto *g = const_cast<TfheHipPublicGallery *>(cg);
    if (!g->img) g->img = Engine::get().upload_public(g->p.N, g->polys.data(), g->R);
    return g->img;
}

// the three broadcast forms: how many products the call makes
int32_t mul_total(const std::string &w, const TfheHipPublicGallery *g, int32_t first, int32_t npolys, int32_t count) {
    if (npolys < 1 || npolys > PUBLIC_MAX_COUNT) api_fail(w + "npolys must be in 1.." + std::to_string(PUBLIC_MAX_COUNT));
    if (count < 1 || count > PUBLIC_MAX_COUNT) api_fail(w + "count must be in 1.." + std::to_string(PUBLIC_MAX_COUNT));
    if (first < 0 || (int64_t)first + npolys > g->R)
        api_fail(w + "poly_index .. poly_index + npolys - 1 must lie in 0.." + std::to_string(g->R - 1));
    if (npolys != 1 && count != 1 && npolys != count) api_fail(w + "npolys and count must be equal unless one of them is 1");
    return npolys > count ? npolys : count;
}

// every argument before the device is looked at, in the order the header lists the refusals
int mul_impl(const char *who, const TfheHipPublicGallery *g, int32_t first, int32_t npolys, const Torus32 *ring, int32_t count,
             Torus32 *out, bool on_device, bool raw) {
    const std::string w = std::string(who) + ": ";
    gallery_checked(w, g);
    if (!ring || !out) api_fail(w + "null ring words or destination");
    const int32_t total = mul_total(w, g, first, npolys, count);
    if (on_device) {
        const uintptr_t rb = reinterpret_cast<uintptr_t>(ring), ob = reinterpret_cast<uintptr_t>(out);
        // (the kernel stores 16 bytes at a time; a workgroup reads its sample while others store)
        if ((rb | ob) & 15) api_fail(w + "device words must be 16-byte aligned");
        const uintptr_t sb = (uintptr_t)2 * g->p.N * 4;
        if (rb < ob + (uintptr_t)total * sb && ob < rb + (uintptr_t)count * sb) api_fail(w + "the destination overlaps the ring words");
    }
    auto lk = recorder_lock();
    if (raw) finish_flight_locked();
    // names no pool slot: what is recorded stays recorded, a flush in flight goes on (the product is ordered behind it on
    // the stream and works in scratch entries of its own)
    const RingImage *img = gallery_image(g);           // out of device memory: ApiError, nothing has changed
    Engine::get().run_public_mul(img, g->p.N, first, npolys == 1 ? 0 : 1, ring, count, total, on_device, out);
    return 0;
}

// what the inner products and their raw rows check alike; returns S
int32_t inner_shape(const std::string &w, const TfheHipPublicGallery *g, int32_t M, int32_t width) {
    const int N = g->p.N;
    if (width < 1 || width > N || (width & (width - 1))) api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
    if (M < 1) api_fail(w + "M must be at least 1");
    const int32_t S = N / width;
    if ((int64_t)M > (int64_t)g->R * S)
        api_fail(w + "M = " + std::to_string(M) + " entries of width " + std::to_string(width) + " need more than the " + std::to_string(g->R) +
                 " polynomials of the gallery");
    return S;
}

int inner_impl(const char *who, const TfheHipPublicGallery *g, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *probe, int32_t M,
               int32_t width, LweSample *result, bool on_device) {
    const std::string w = std::string(who) + ": ";
    if (!probe || !result) api_fail(w + "null ring words or result");
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    gallery_checked(w, g);
    const Params &p = bk->bk->p;
    if (p.N != g->p.N || p.k != g->p.k) api_fail(w + "the gallery and the cloud key belong to different rings");
    inner_shape(w, g, M, width);
    if (on_device && (reinterpret_cast<uintptr_t>(probe) & 15)) api_fail(w + "device words must be 16-byte aligned");
    auto lk = recorder_lock();
    // as the unpack: every result ours, of the key's LWE dimension, not bound to the pool of another shape
    check_runs(w, UNPACK_RESULT, ResultsView(result), M, p);
    SlotPool *pool = pool_of_key(bk);
    // a flush in flight owns the key switch's partial sums; what is recorded and has not run stays recorded
    finish_flight_locked();
    const RingImage *img = gallery_image(g);           // out of device memory: ApiError, nothing has changed
    import_into_fresh_slots(pool, ResultsView(result), M, [&](const int32_t *slots) {
        Engine::get().run_public_inner(img, g->p, bk->bk->dev, probe, on_device, M, width, pool, slots, nullptr, !on_device);
    });
    return 0;
}

// ---- sums over several ring samples (ring_public.hpp "sums of products over several ring samples") ----
// terms and the gallery read as groups of them
void sum_terms_checked(const std::string &w, const TfheHipPublicGallery *g, int32_t terms) {
    if (terms < 1 || terms > PUBLIC_MAX_TERMS) api_fail(w + "terms must be in 1.." + std::to_string(PUBLIC_MAX_TERMS));
    if (g->R % terms) api_fail(w + "the gallery's " + std::to_string(g->R) + " polynomials are not a multiple of terms = " + std::to_string(terms));
}
// the CRT bound of the `ngroups` groups from polynomial first_poly on, before the device is looked at; the first offending
// group is named
void sum_crt_checked(const std::string &w, const TfheHipPublicGallery *g, int32_t terms, int64_t first_poly, int64_t ngroups) {
    for (int64_t grp = 0; grp < ngroups; ++grp) {
        int64_t sum = 0;
        for (int t = 0; t < terms; ++t) sum += g->maxabs[(size_t)(first_poly + grp * terms + t)];
        if (!public_sum_crt_ok(g->p.N, terms, sum))
            api_fail(w + "group " + std::to_string(grp) + " (polynomials " + std::to_string(first_poly + grp * terms) + ".." +
                     std::to_string(first_poly + grp * terms + terms - 1) + "): its terms' largest coefficients sum to " + std::to_string(sum) +
                     ", past " + std::to_string(public_max_coef(g->p.N)) + ", the exact range of the two-prime CRT (ring_public.hpp CRT bound)");
    }
}

int sum_mul_impl(const char *who, const TfheHipPublicGallery *g, int32_t first, int32_t terms, int32_t ngroups, const Torus32 *ring,
                 Torus32 *out, bool on_device, bool raw) {
    const std::string w = std::string(who) + ": ";
    gallery_checked(w, g);
    if (!ring || !out) api_fail(w + "null ring words or destination");
    sum_terms_checked(w, g, terms);
    if (ngroups < 1 || ngroups > PUBLIC_MAX_COUNT) api_fail(w + "ngroups must be in 1.." + std::to_string(PUBLIC_MAX_COUNT));
    if (first < 0 || (int64_t)first + (int64_t)ngroups * terms > g->R)
        api_fail(w + "poly_index .. poly_index + ngroups terms - 1 must lie in 0.." + std::to_string(g->R - 1));
    sum_crt_checked(w, g, terms, first, ngroups);
    if (on_device) {
        const uintptr_t rb = reinterpret_cast<uintptr_t>(ring), ob = reinterpret_cast<uintptr_t>(out);
        if ((rb | ob) & 15) api_fail(w + "device words must be 16-byte aligned");
        const uintptr_t sb = (uintptr_t)2 * g->p.N * 4;
        if (rb < ob + (uintptr_t)ngroups * sb && ob < rb + (uintptr_t)terms * sb) api_fail(w + "the destination overlaps the ring words");
    }
    auto lk = recorder_lock();
    if (raw) finish_flight_locked();
    // as tfhe_hip_ring_mul_public: names no pool slot, what is recorded stays recorded, a flush in flight goes on
    const RingImage *img = gallery_image(g);           // out of device memory: ApiError, nothing has changed
    Engine::get().run_public_sum_mul(img, g->p.N, first, terms, ngroups, ring, on_device, out);
    return 0;
}

// what the summed inner products and their raw rows check alike
void sum_inner_shape(const std::string &w, const TfheHipPublicGallery *g, int32_t terms, int32_t M, int32_t width) {
    const int N = g->p.N;
    sum_terms_checked(w, g, terms);
    if (width < 1 || width > N || (width & (width - 1))) api_fail(w + "width must be a power of two in 1.." + std::to_string(N));
    if (M < 1) api_fail(w + "M must be at least 1");
    const int64_t S = N / width, groups = g->R / terms;
    if ((int64_t)M > groups * S)
        api_fail(w + "M = " + std::to_string(M) + " entries of width " + std::to_string(width) + " need more than the " + std::to_string(groups) +
                 " groups of the gallery");
    sum_crt_checked(w, g, terms, 0, (M + S - 1) / S);
}

int sum_inner_impl(const char *who, const TfheHipPublicGallery *g, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *probe,
                   int32_t terms, int32_t M, int32_t width, LweSample *result, bool on_device) {
    const std::string w = std::string(who) + ": ";
    if (!probe || !result) api_fail(w + "null ring words or result");
    if (!bk || !bk->bk) api_fail(w + "null cloud key");
    gallery_checked(w, g);
    const Params &p = bk->bk->p;
    if (p.N != g->p.N || p.k != g->p.k) api_fail(w + "the gallery and the cloud key belong to different rings");
    sum_inner_shape(w, g, terms, M, width);
    if (on_device && (reinterpret_cast<uintptr_t>(probe) & 15)) api_fail(w + "device words must be 16-byte aligned");
    auto lk = recorder_lock();
    check_runs(w, UNPACK_RESULT, ResultsView(result), M, p);
    SlotPool *pool = pool_of_key(bk);
    // a flush in flight owns the key switch's partial sums; what is recorded and has not run stays recorded
    finish_flight_locked();
    const RingImage *img = gallery_image(g);           // out of device memory: ApiError, nothing has changed
    import_into_fresh_slots(pool, ResultsView(result), M, [&](const int32_t *slots) {
        Engine::get().run_public_sum_inner(img, g->p, bk->bk->dev, terms, probe, on_device, M, width, pool, slots, nullptr, !on_device);
    });
    return 0;
}

}  // namespace

extern "C" {

TfheHipPublicGallery *tfhe_hip_new_public_gallery(const TFheGateBootstrappingParameterSet *params, const int32_t *polys, int32_t R) {
    const std::string w = "tfhe_hip_new_public_gallery: ";
    // every argument before the device is looked at: a refusal has no effect
    if (!params || !params->in_out_params) { set_error(w + "null parameter set"); return nullptr; }
    const Params &p = params_of(params);
    if ((p.N != 1024 && p.N != 2048) || p.k != 1) { set_error(w + "the product kernel is built for N = 1024 or 2048 and k = 1"); return nullptr; }
    if (R < 1 || R > PUBLIC_MAX_POLYS) { set_error(w + "R must be in 1.." + std::to_string(PUBLIC_MAX_POLYS)); return nullptr; }
    if (!polys) { set_error(w + "null polynomials"); return nullptr; }
    const int64_t T = public_max_coef(p.N), words = (int64_t)R * p.N;
    for (int64_t j = 0; j < words; ++j)
        if (polys[j] > T || polys[j] < -T) {
            set_error(w + "coefficient " + std::to_string(polys[j]) + " at index " + std::to_string(j) + " (polynomial " + std::to_string(j / p.N) +
                      ", coefficient " + std::to_string(j % p.N) + ") is outside -" + std::to_string(T) + ".." + std::to_string(T) +
                      ", the exact range of the two-prime CRT (ring_public.hpp CRT bound)");
            return nullptr;
        }
    std::vector<int32_t> maxabs((size_t)R, 0);
    for (int64_t j = 0; j < words; ++j) maxabs[j / p.N] = std::max(maxabs[j / p.N], polys[j] < 0 ? -polys[j] : polys[j]);
    return new TfheHipPublicGallery{PUBLIC_MAGIC, p, R, std::vector<int32_t>(polys, polys + words), nullptr, std::move(maxabs)};
}
void tfhe_hip_delete_public_gallery(TfheHipPublicGallery *g) {
    if (!g) return;
    if (g->magic != PUBLIC_MAGIC) { set_error("tfhe_hip_delete_public_gallery: not a gallery (or already deleted)"); return; }
    auto lk = recorder_lock();
    Engine::get().free_public(g->img);                           // (waits for the stream: a product in flight reads the image)
    g->magic = 0;
    delete g;
}
int32_t tfhe_hip_public_gallery_polys(const TfheHipPublicGallery *g) {
    if (!g || g->magic != PUBLIC_MAGIC) { set_error("tfhe_hip_public_gallery_polys: null or deleted gallery"); return -1; }
    return g->R;
}

int tfhe_hip_ring_mul_public(const TfheHipPublicGallery *g, int32_t poly_index, int32_t npolys, const Torus32 *ring_words, int32_t count,
                             Torus32 *out_ring_words) {
    return guarded_rc([&] { return mul_impl("tfhe_hip_ring_mul_public", g, poly_index, npolys, ring_words, count, out_ring_words, false, false); });
}
int tfhe_hip_ring_mul_public_device(const TfheHipPublicGallery *g, int32_t poly_index, int32_t npolys, const void *device_ring_words,
                                    int32_t count, void *device_out) {
    return guarded_rc([&] {
        return mul_impl("tfhe_hip_ring_mul_public_device", g, poly_index, npolys, static_cast<const Torus32 *>(device_ring_words), count,
                        static_cast<Torus32 *>(device_out), true, false);
    });
}

int tfhe_hip_ring_inner_public(const TfheHipPublicGallery *g, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *probe_ring_words,
                               int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] { return inner_impl("tfhe_hip_ring_inner_public", g, bk, probe_ring_words, M, width, result, false); });
}
int tfhe_hip_ring_inner_public_device(const TfheHipPublicGallery *g, const TFheGateBootstrappingCloudKeySet *bk,
                                      const void *device_probe_ring_words, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] {
        return inner_impl("tfhe_hip_ring_inner_public_device", g, bk, static_cast<const Torus32 *>(device_probe_ring_words), M, width, result,
                          true);
    });
}

int tfhe_hip_kernel_ring_public_product(const TfheHipPublicGallery *g, int32_t poly_index, int32_t npolys, const Torus32 *ring_words,
                                        int32_t count, Torus32 *out_words) {
    return guarded_rc([&] { return mul_impl("tfhe_hip_kernel_ring_public_product", g, poly_index, npolys, ring_words, count, out_words, false, true); });
}
int tfhe_hip_kernel_ring_public_rows(const TfheHipPublicGallery *g, const Torus32 *probe_ring_words, int32_t M, int32_t width,
                                     Torus32 *out_rows) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_ring_public_rows: ";
        gallery_checked(w, g);
        if (!probe_ring_words || !out_rows) api_fail(w + "null argument");
        inner_shape(w, g, M, width);
        auto lk = recorder_lock();
        finish_flight_locked();                                  // (the row buffer is the unpack's)
        const RingImage *img = gallery_image(g);
        Engine::get().run_public_inner(img, g->p, nullptr, probe_ring_words, false, M, width, nullptr, nullptr, out_rows, true);
        return 0;
    });
}

int tfhe_hip_test_public_bounds(int32_t N, int32_t T) {
    if ((N != 1024 && N != 2048) || T < 1) {
        set_error("test_public_bounds: bad arguments");
        return -1;
    }
    return public_crt_ok(N, T) ? 0 : 1;
}

int tfhe_hip_ring_mul_public_sum(const TfheHipPublicGallery *g, int32_t poly_index, int32_t terms, int32_t ngroups, const Torus32 *ring_words,
                                 Torus32 *out_ring_words) {
    return guarded_rc([&] { return sum_mul_impl("tfhe_hip_ring_mul_public_sum", g, poly_index, terms, ngroups, ring_words, out_ring_words, false, false); });
}
int tfhe_hip_ring_mul_public_sum_device(const TfheHipPublicGallery *g, int32_t poly_index, int32_t terms, int32_t ngroups,
                                        const void *device_ring_words, void *device_out) {
    return guarded_rc([&] {
        return sum_mul_impl("tfhe_hip_ring_mul_public_sum_device", g, poly_index, terms, ngroups, static_cast<const Torus32 *>(device_ring_words),
                            static_cast<Torus32 *>(device_out), true, false);
    });
}
int tfhe_hip_ring_inner_public_sum(const TfheHipPublicGallery *g, const TFheGateBootstrappingCloudKeySet *bk, const Torus32 *probe_ring_words,
                                   int32_t terms, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] { return sum_inner_impl("tfhe_hip_ring_inner_public_sum", g, bk, probe_ring_words, terms, M, width, result, false); });
}
int tfhe_hip_ring_inner_public_sum_device(const TfheHipPublicGallery *g, const TFheGateBootstrappingCloudKeySet *bk,
                                          const void *device_probe_ring_words, int32_t terms, int32_t M, int32_t width, LweSample *result) {
    return guarded_rc([&] {
        return sum_inner_impl("tfhe_hip_ring_inner_public_sum_device", g, bk, static_cast<const Torus32 *>(device_probe_ring_words), terms, M,
                              width, result, true);
    });
}
int tfhe_hip_kernel_ring_public_sum_product(const TfheHipPublicGallery *g, int32_t poly_index, int32_t terms, int32_t ngroups,
                                            const Torus32 *ring_words, Torus32 *out_words) {
    return guarded_rc(
        [&] { return sum_mul_impl("tfhe_hip_kernel_ring_public_sum_product", g, poly_index, terms, ngroups, ring_words, out_words, false, true); });
}
int tfhe_hip_kernel_ring_public_sum_rows(const TfheHipPublicGallery *g, const Torus32 *probe_ring_words, int32_t terms, int32_t M,
                                         int32_t width, Torus32 *out_rows) {
    return guarded_rc([&] {
        const std::string w = "tfhe_hip_kernel_ring_public_sum_rows: ";
        gallery_checked(w, g);
        if (!probe_ring_words || !out_rows) api_fail(w + "null argument");
        sum_inner_shape(w, g, terms, M, width);
        auto lk = recorder_lock();
        finish_flight_locked();                                  // (the row buffer is the unpack's)
        const RingImage *img = gallery_image(g);
        Engine::get().run_public_sum_inner(img, g->p, nullptr, terms, probe_ring_words, false, M, width, nullptr, nullptr, out_rows, true);
        return 0;
    });
}

int tfhe_hip_test_public_sum_bounds(int32_t N, int32_t terms, int64_t coef_sum) {
    if ((N != 1024 && N != 2048) || terms < 1 || terms > PUBLIC_MAX_TERMS || coef_sum < 0) {
        set_error("test_public_sum_bounds: bad arguments");
        return -1;
    }
    return public_sum_crt_ok(N, terms, coef_sum) ? 0 : 1;
}

}  // extern "C"
