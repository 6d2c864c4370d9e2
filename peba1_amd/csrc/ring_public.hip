// ring_public.hip -- a ring sample times public small-integer polynomials on gfx950 (ring_public.hpp has the definition
// and the bounds).
//
//   public_image_kernel  one wave64 per polynomial and prime: the coefficients (|q| <= 2^11, the digit bound) go through one
//                        forward NTT, are canonicalised and scaled, and are stored in the order a lane of the product
//                        kernel fetches them with 16-byte loads.  Once per gallery object.
//   public_kernel        one workgroup of two wave64 per pair of a ring sample and a public polynomial; wave p works modulo
//                        prime p.  Per polynomial u of the sample: each lane loads its words, reduces them below P (one
//                        Montgomery product with R mod P), one forward NTT, ONE product per coefficient with the image word,
//                        its Montgomery reduction, one inverse NTT; the residues go to LDS in natural order.  Wave p then
//                        owns output polynomial p: it reads four consecutive coefficients of both primes, applies the
//                        signed CRT and, in the raw form, writes 16 bytes per lane and store.  With rows the torus words go
//                        back into LDS over prime 0's residues (every lane overwrites the 16 bytes it alone has just
//                        read), one more barrier, and the two waves write the rows Extract_(e w), e < S = N / w, in
//                        ring_extract_kernel's layout (unpack.hip), as cmux.hip's inner_kernel writes them: a lane owns
//                        16-byte groups of a row, reads the mask polynomial descending from A[e w - 4g] in LDS and stores
//                        16 bytes; the last group is (B[e w], 0, 0, 0).  Only rows below M are written.
//                        4 forward and 4 inverse wave transforms a workgroup (2 + 2 a wave), where inner_kernel takes
//                        4 l forward and 4 inverse; no 64-bit accumulator lives across a transform.
// No atomics, no global scratch beyond the row buffer; a workgroup reads nothing another workgroup of the launch writes.
//
// kernels.hip is not touched by this file; the few lines it keeps private (the per-prime context) are restated once, in
// ring_wave.hpp (through ring_public.hpp), with the tail public_kernel shares with cmux.hip's inner_kernel.
#include "ring_public.hpp"

namespace tfhe_hip {

namespace {

// grid (count, 2 primes), one wave each
template <int LOGN>
__global__ __launch_bounds__(64) void public_image_kernel(PublicImageArgs a) {
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t scr[NTT::SCRATCH_WORDS];
    const int lane = threadIdx.x;
    const int p = blockIdx.y;
    const int poly = blockIdx.x;                                 // < a.count: the grid is a.count polynomials wide
    const PrimeCtx c = ring_prime_ctx(p, a.tw, N);
    const uint32_t scale = p ? a.scale[1] : a.scale[0];
    const int32_t *src = a.polys + (size_t)poly * N;
    int32_t x[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) x[r] = src[r * 64 + lane];    // |x| <= 2^11 (the constructor's check)
    NTT::forward(x, c, scr, lane);                               // |x| < 6.1 P / 6.7 P
    uint4 *dst = reinterpret_cast<uint4 *>(a.img + ((size_t)poly * 2 + p) * N) + lane;
#pragma unroll
    for (int g = 0; g < REGS / 4; ++g) {
        uint32_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            int32_t m = x[4 * g + e] % (int32_t)c.P;
            if (m < 0) m += (int32_t)c.P;
            v[e] = (uint32_t)((uint64_t)(uint32_t)m * scale % c.P);
        }
        dst[g * 64] = make_uint4(v[0], v[1], v[2], v[3]);
    }
}

static_assert(public_product_ok(1024) && public_product_ok(2048), "one product, one reduction, then the inverse transform");

template <int LOGN>
__global__ __launch_bounds__(128) void public_kernel(PublicArgs a) {
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t lds_scr[2][NTT::SCRATCH_WORDS];
    // residues in natural order, [prime = the wave that wrote them][output polynomial][N]
    __shared__ __align__(16) uint32_t lds_x[2][2][N];
    const int tid = threadIdx.x;
    const int p = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const PrimeCtx c = ring_prime_ctx(p, a.tw, N);
    uint32_t *scr = lds_scr[p];

    const int wg = blockIdx.x;                                   // < a.count: the grid is a.count workgroups
    const int32_t *ring = a.ring + (size_t)wg * a.ring_stride;
    // image of this workgroup's polynomial: [prime][N], a lane's registers of layout L2 as 16-byte groups
    const uint4 *img = reinterpret_cast<const uint4 *>(a.img + (((size_t)wg * a.img_step) * 2 + p) * N) + lane;
    typename NTT::FwdTw0 t0;                 // lane-uniform and the same for both transforms
    t0.load(c, lane);
    uint4 b[REGS / 4];
#pragma unroll
    for (int g = 0; g < REGS / 4; ++g) b[g] = img[g * 64];

    for (int u = 0; u < 2; ++u) {
        // coefficient j = 64 r + lane of polynomial u (layout L0 of ntt_wave.hpp), reduced: |x| < P
        int32_t x[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) x[r] = mont_mul(ring[u * N + r * 64 + lane], c.rmod, c.P, c.pinv);
        NTT::template forward<false>(x, c, scr, lane, t0);       // |x| < 7.6 P / 8.2 P (ring_public.hpp)
        // |x w| < 8.2 P^2 -> reduction below 0.76 P (product bound) -> inverse NTT: signed residues below P, natural order
#pragma unroll
        for (int g = 0; g < REGS / 4; ++g) {
            x[4 * g + 0] = mont_redc((int64_t)x[4 * g + 0] * (int32_t)b[g].x, c.P, c.pinv);
            x[4 * g + 1] = mont_redc((int64_t)x[4 * g + 1] * (int32_t)b[g].y, c.P, c.pinv);
            x[4 * g + 2] = mont_redc((int64_t)x[4 * g + 2] * (int32_t)b[g].z, c.P, c.pinv);
            x[4 * g + 3] = mont_redc((int64_t)x[4 * g + 3] * (int32_t)b[g].w, c.P, c.pinv);
        }
        NTT::inverse(x, c, scr, lane);
#pragma unroll
        for (int r = 0; r < REGS; ++r) lds_x[p][u][r * 64 + lane] = (uint32_t)x[r];
    }
    // the waves took different primes and now exchange through LDS alone: the barrier form ntt_wave.hpp documents for
    // that (both waves reach it on the same path; nothing was stored to global memory yet)
    lds_barrier();
    ring_crt_rows<LOGN>(lds_x, p, lane, tid, wg, a.out, a.rows);    // the CRT, the full product, the rows (ring_wave.hpp)
}

}  // namespace

InvPlanWords inv_plan_words(int logn) {
    const InvPlan pl = make_inv_plan(logn);
    InvPlanWords w{};
    w.nsteps = pl.nsteps;
    for (int k = 0; k < 12; ++k) { w.fan[k] = pl.fan[k]; w.renorm[k] = pl.renorm[k] ? 1 : 0; }
    w.out_bound = pl.out_bound;
    return w;
}

bool launch_public_image(hipStream_t s, const PublicImageArgs &a) {
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > PUBLIC_MAX_POLYS || !a.polys || !a.img || !a.tw ||
        (reinterpret_cast<uintptr_t>(a.img) & 15u))
        return false;
    if (a.N == 2048) hipLaunchKernelGGL((public_image_kernel<11>), dim3(a.count, 2), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((public_image_kernel<10>), dim3(a.count, 2), dim3(64), 0, s, a);
    return true;
}

bool launch_public(hipStream_t s, const PublicArgs &a) {
    const RingRows &t = a.rows;
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > PUBLIC_MAX_COUNT || (a.img_step != 0 && a.img_step != 1) ||
        (a.ring_stride != 0 && (a.ring_stride < 2 * (int64_t)a.N || (a.ring_stride & 3))) || !a.ring || !a.img || !a.tw ||
        (!a.out && !t.u_buf) || ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.img)) & 15u))
        return false;
    if (t.u_buf && (ring_rows_error(a.N, a.count, t.M, t.width, t.u_stride) || (reinterpret_cast<uintptr_t>(t.u_buf) & 15u))) return false;
    if (a.N == 2048) hipLaunchKernelGGL((public_kernel<11>), dim3(a.count), dim3(128), 0, s, a);
    else hipLaunchKernelGGL((public_kernel<10>), dim3(a.count), dim3(128), 0, s, a);
    return true;
}

}  // namespace tfhe_hip
