// ring_public_sum.hip -- sums of public-polynomial products over several ring samples on gfx950 (ring_public.hpp has the
// definition and the bounds; include/tfhe_hip.h "public products over several ring samples").
//
//   public_sum_kernel    one workgroup of two wave64 per output group g; wave p works modulo prime p, as public_kernel
//                        does.  Per output polynomial u and term t < K: each lane loads its words of c_t[u], reduces them
//                        below P (one Montgomery product with R mod P), one forward NTT, one product per coefficient with
//                        the image word of polynomial g K + t, ADDED into a 64-bit accumulator.  Then ONE Montgomery
//                        reduction and ONE inverse NTT per u; the residues go to LDS in natural order and the tail is
//                        public_kernel's (ring_wave.hpp ring_crt_rows): the signed CRT, then the full sum or the rows
//                        Extract_(e w).  u is the outer loop, so one polynomial's accumulator is live at a time:
//                        2 K forward and 2 inverse wave transforms a wave, where K launches of public_kernel take
//                        2 K + 2 K.  K = 1 computes public_kernel's words: one product, the same reduction.
// No atomics, no global scratch beyond the row buffer; a workgroup reads nothing another workgroup of the launch writes.
//
// A translation unit of its own: ring_public.hip and the listings of its kernels stay what they were.
#include "ring_public.hpp"

namespace tfhe_hip {

namespace {

static_assert(public_sum_mac_ok(1024, PUBLIC_MAX_TERMS) && public_sum_mac_ok(2048, PUBLIC_MAX_TERMS),
              "PUBLIC_MAX_TERMS products, one reduction, then the inverse transform");

template <int LOGN>
__global__ __launch_bounds__(128) void public_sum_kernel(PublicSumArgs a) {
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
    // images of this workgroup's group, polynomial wg terms + t at step 2N words: [prime][N], 16-byte groups of layout L2
    const uint4 *img = reinterpret_cast<const uint4 *>(a.img + (((size_t)wg * a.terms) * 2 + p) * N) + lane;
    typename NTT::FwdTw0 t0;                 // lane-uniform and the same for every transform
    t0.load(c, lane);

    // u outermost: one polynomial's accumulator is live at a time
    for (int u = 0; u < 2; ++u) {
        int64_t acc[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) acc[r] = 0;
        for (int t = 0; t < a.terms; ++t) {
            const int32_t *ring = a.ring + ((size_t)t * 2 + u) * N;
            const uint4 *bp = img + (size_t)t * (N / 2);         // 2N words a polynomial = N / 2 uint4
            // coefficient j = 64 r + lane of polynomial u of sample t (layout L0 of ntt_wave.hpp), reduced: |x| < P
            int32_t x[REGS];
#pragma unroll
            for (int r = 0; r < REGS; ++r) x[r] = mont_mul(ring[r * 64 + lane], c.rmod, c.P, c.pinv);
            NTT::template forward<false>(x, c, scr, lane, t0);   // |x| < 7.6 P / 8.2 P (ring_public.hpp)
#pragma unroll
            for (int g = 0; g < REGS / 4; ++g) {
                const uint4 b = bp[g * 64];
                acc[4 * g + 0] += (int64_t)x[4 * g + 0] * (int32_t)b.x;
                acc[4 * g + 1] += (int64_t)x[4 * g + 1] * (int32_t)b.y;
                acc[4 * g + 2] += (int64_t)x[4 * g + 2] * (int32_t)b.z;
                acc[4 * g + 3] += (int64_t)x[4 * g + 3] * (int32_t)b.w;
            }
        }
        // |acc| < terms 8.2 P^2 -> reduction below 4 P (MAC bound) -> inverse NTT: signed residues below P, natural order
        int32_t y[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) y[r] = mont_redc(acc[r], c.P, c.pinv);
        NTT::inverse(y, c, scr, lane);
#pragma unroll
        for (int r = 0; r < REGS; ++r) lds_x[p][u][r * 64 + lane] = (uint32_t)y[r];
    }
    // the waves took different primes and now exchange through LDS alone: the barrier form ntt_wave.hpp documents for
    // that (both waves reach it on the same path; nothing was stored to global memory yet)
    lds_barrier();
    ring_crt_rows<LOGN>(lds_x, p, lane, tid, wg, a.out, a.rows);    // the CRT, the full sum, the rows (ring_wave.hpp)
}

}  // namespace

bool launch_public_sum(hipStream_t s, const PublicSumArgs &a) {
    const RingRows &t = a.rows;
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > PUBLIC_MAX_COUNT || a.terms < 1 || a.terms > PUBLIC_MAX_TERMS ||
        !public_sum_mac_ok(a.N, a.terms) || !a.ring || !a.img || !a.tw || (!a.out && !t.u_buf) ||
        ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.img) | reinterpret_cast<uintptr_t>(a.ring)) & 15u))
        return false;
    if (t.u_buf && (ring_rows_error(a.N, a.count, t.M, t.width, t.u_stride) || (reinterpret_cast<uintptr_t>(t.u_buf) & 15u))) return false;
    if (a.N == 2048) hipLaunchKernelGGL((public_sum_kernel<11>), dim3(a.count), dim3(128), 0, s, a);
    else hipLaunchKernelGGL((public_sum_kernel<10>), dim3(a.count), dim3(128), 0, s, a);
    return true;
}

}  // namespace tfhe_hip
