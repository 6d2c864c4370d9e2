// ring_inner_sum.hip -- sums of TGSW products over several ring samples on gfx950 (ring_inner_sum.hpp has the definition
// and the two bounds; include/tfhe_hip.h "TGSW products over several ring samples").
//
//   inner_sum_kernel     one workgroup of two wave64 per output group g; wave q works modulo prime q, as inner_kernel
//                        (cmux.hip) does.  Per term t < K and input polynomial u: each lane loads its coefficients of
//                        c_(gK+t)[u] (+ the decomposition's offset) once, then for each of the l digits one forward NTT of
//                        the signed digit polynomial and a 64-bit multiply-accumulate against the two output polynomials
//                        of row (u, p) of selector sample b + t -- all terms into the SAME two accumulators.  After every
//                        `block` rows the accumulators are folded in place (one Montgomery reduction and one product with
//                        R mod P a register: ring_inner_sum.hpp MAC bound); the branch is workgroup-uniform and holds no
//                        barrier.  After the K (k+1) l rows one Montgomery reduction and inverse NTT per output
//                        polynomial; the residues go to LDS in natural order and the tail is inner_kernel's
//                        (ring_wave.hpp ring_crt_rows): the signed CRT, then the full sum or the rows Extract_(e w).
//                        K (k+1) l forward and 2 inverse wave transforms a wave, where K launches of inner_kernel take
//                        K (k+1) l + 2 K, K CRTs and K extractions.  K = 1 never folds and computes inner_kernel's words.
// No atomics, no global scratch beyond the row buffer; a workgroup reads nothing another workgroup of the launch writes.
//
// A translation unit of its own: cmux.hip, cmux_body.inc and the listings of their kernels stay what they were.
#include "ring_inner_sum.hpp"

namespace tfhe_hip {

namespace {

template <int LOGN>
__global__ __launch_bounds__(128) void inner_sum_kernel(InnerSumArgs x) {
    const CmuxArgs &a = x.c;
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t lds_scr[2][NTT::SCRATCH_WORDS];
    // residues in natural order, [prime = the wave that wrote them][output polynomial][N]
    __shared__ __align__(16) uint32_t lds_x[2][2][N];
    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const PrimeCtx c = ring_prime_ctx(q, a.tw, N);
    uint32_t *scr = lds_scr[q];

    const int wg = blockIdx.x;                                   // < a.count: the grid is a.count workgroups
    const int32_t *ring = a.d0 + (size_t)wg * a.stride;          // the group's `terms` samples, 2N words each
    const uint32_t mask = (1u << a.Bgbit) - 1u;
    const int32_t half = 1 << (a.Bgbit - 1);
    typename NTT::FwdTw0 t0;                 // lane-uniform and the same for every transform
    t0.load(c, lane);

    int64_t acc0[REGS], acc1[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) { acc0[r] = 0; acc1[r] = 0; }
    // image of row (sample, u, p): [X = sample (k+1) l + u l + p][prime][polynomial 2][N] (kernels.hip bk_transform_kernel,
    // nw = 2): the rows of samples a.bit .. a.bit + terms - 1 are consecutive, row X = t (k+1) l + u l + p from the first
    const uint4 *rowimg = reinterpret_cast<const uint4 *>(a.img + ((size_t)a.bit * 2 * a.l * 2 + q) * 2 * N) + lane;
    int inblock = 0;                                             // rows since the last fold; workgroup-uniform
    for (int t = 0; t < x.terms; ++t) {
        for (int u = 0; u < 2; ++u) {
            // coefficient j = 64 r + lane of polynomial u of sample t (layout L0 of ntt_wave.hpp)
            uint32_t v[REGS];
#pragma unroll
            for (int r = 0; r < REGS; ++r) v[r] = (uint32_t)ring[((size_t)t * 2 + u) * N + r * 64 + lane] + a.offset;
            for (int p = 0; p < a.l; ++p) {
                if (inblock == x.block) {
                    // the fold: the same residues, |acc| < 4 P R (ring_inner_sum.hpp MAC bound)
#pragma unroll
                    for (int r = 0; r < REGS; ++r) {
                        acc0[r] = (int64_t)mont_redc(acc0[r], c.P, c.pinv) * (int64_t)(int32_t)c.rmod;
                        acc1[r] = (int64_t)mont_redc(acc1[r], c.P, c.pinv) * (int64_t)(int32_t)c.rmod;
                    }
                    inblock = 0;
                }
                ++inblock;
                const int shift = 32 - (p + 1) * a.Bgbit;
                int32_t d[REGS];
#pragma unroll
                for (int r = 0; r < REGS; ++r) d[r] = (int32_t)((v[r] >> shift) & mask) - half;    // |d| <= Bg/2 <= 2^11
                NTT::template forward<false>(d, c, scr, lane, t0);          // |d| < 6.1 P / 6.7 P (cmux.hpp)
                const uint4 *bp = rowimg + (size_t)((t * 2 + u) * a.l + p) * N;   // 4N words per row = N uint4
#pragma unroll
                for (int g = 0; g < REGS / 4; ++g) {
                    const uint4 b0 = bp[g * 64], b1 = bp[N / 4 + g * 64];
                    acc0[4 * g + 0] += (int64_t)d[4 * g + 0] * (int32_t)b0.x;
                    acc0[4 * g + 1] += (int64_t)d[4 * g + 1] * (int32_t)b0.y;
                    acc0[4 * g + 2] += (int64_t)d[4 * g + 2] * (int32_t)b0.z;
                    acc0[4 * g + 3] += (int64_t)d[4 * g + 3] * (int32_t)b0.w;
                    acc1[4 * g + 0] += (int64_t)d[4 * g + 0] * (int32_t)b1.x;
                    acc1[4 * g + 1] += (int64_t)d[4 * g + 1] * (int32_t)b1.y;
                    acc1[4 * g + 2] += (int64_t)d[4 * g + 2] * (int32_t)b1.z;
                    acc1[4 * g + 3] += (int64_t)d[4 * g + 3] * (int32_t)b1.w;
                }
            }
        }
    }
    // |acc| < (block f + 0.102) P^2 -> reduction below 4 P (MAC bound) -> inverse NTT: signed residues below P, natural order
    int32_t y[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) y[r] = mont_redc(acc0[r], c.P, c.pinv);
    NTT::inverse(y, c, scr, lane);
#pragma unroll
    for (int r = 0; r < REGS; ++r) lds_x[q][0][r * 64 + lane] = (uint32_t)y[r];
#pragma unroll
    for (int r = 0; r < REGS; ++r) y[r] = mont_redc(acc1[r], c.P, c.pinv);
    NTT::inverse(y, c, scr, lane);
#pragma unroll
    for (int r = 0; r < REGS; ++r) lds_x[q][1][r * 64 + lane] = (uint32_t)y[r];
    // the waves took different primes and now exchange through LDS alone: the barrier form ntt_wave.hpp documents for
    // that (both waves reach it on the same path; nothing was stored to global memory yet)
    lds_barrier();
    ring_crt_rows<LOGN>(lds_x, q, lane, tid, wg, a.out, x.rows);    // the CRT, the full sum, the rows (ring_wave.hpp)
}

}  // namespace

bool launch_inner_sum(hipStream_t s, const InnerSumArgs &x) {
    const CmuxArgs &a = x.c;
    const RingRows &t = x.rows;
    // the gadget as launch_inner, then the two bounds of the sum; the operands are 16-byte aligned like every destination
    if (cmux_gadget_error(a.N, 1, a.l, a.Bgbit) || x.terms < 1 || x.terms > inner_sum_max_terms(a.N, a.l, a.Bgbit) ||
        x.block != inner_sum_block_rows(a.N) || a.bit < 0 || a.bit + x.terms > SELECT_MAX_BITS || a.count < 1 || a.count > INNER_SUM_MAX_GROUPS ||
        a.stride < (int64_t)x.terms * 2 * a.N || (a.stride & 3) || !a.d0 || !a.img || !a.tw || a.d1 || a.rot || a.n_d1 || (!a.out && !t.u_buf) ||
        ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.d0)) & 15u))
        return false;
    if (t.u_buf && (ring_rows_error(a.N, a.count, t.M, t.width, t.u_stride) || (reinterpret_cast<uintptr_t>(t.u_buf) & 15u))) return false;
    if (a.N == 2048) hipLaunchKernelGGL((inner_sum_kernel<11>), dim3(a.count), dim3(128), 0, s, x);
    else hipLaunchKernelGGL((inner_sum_kernel<10>), dim3(a.count), dim3(128), 0, s, x);
    return true;
}

}  // namespace tfhe_hip
