// ring_rotate.hip -- the blind rotation of an encrypted ring sample by an LWE sample on gfx950 (ring_rotate.hpp has the
// definition and the bounds argument; include/tfhe_hip.h "ring LUT bootstrap").
//
//   ring_rotate_kernel   one workgroup of two wave64 per rotation; wave q works modulo prime q, as cmux_kernel (cmux.hip)
//                        does, and the n CMUX steps stay inside the one launch.  Prologue: the 128 threads switch the LWE
//                        sample's n + 1 words to Z_2N (16-bit words in LDS), then wave q writes polynomial q of
//                        ACC_0 = X^(-bbar) c into the accumulator, which lives in LDS as plain torus words for all n
//                        steps.  Per step with abar != 0 (workgroup-uniform; abar = 0 is skipped) and input polynomial
//                        u: each lane reads its coefficients of X^(abar) ACC[u] - ACC[u] (+ the decomposition's offset)
//                        from LDS, then for each of the l digits one forward NTT of the signed digit polynomial and a
//                        64-bit multiply-accumulate against the two output polynomials of row (i, u, p) of the cloud
//                        key's image.  After the (k+1) l rows one Montgomery reduction and inverse NTT per output
//                        polynomial; the residues go to LDS in natural order, a barrier, then wave q owns output
//                        polynomial q: four consecutive coefficients of both primes, the signed CRT, added to ACC[q] in
//                        LDS, 16 bytes per lane and access; a second barrier ends the step (the next one reads both
//                        polynomials, and overwrites the residues).  These are cmux_body.inc's statements with another
//                        operand load and an LDS destination.
//   <., false>           epilogue: wave q writes polynomial q of ACC_n, 16 bytes per lane and store.
//   <., true>            epilogue: the row Extract_0(ACC_n) in ring_extract_kernel's layout (unpack.hip) -- a lane owns
//                        16-byte groups of the row, reads the mask polynomial descending from A[0], negated past the
//                        wrap; the last group is (B[0], 0, 0, 0).
// No atomics, no global scratch; a rotation reads nothing another rotation of the launch writes.
//
// A translation unit of its own: kernels.hip, cmux.hip, cmux_body.inc and the listings of their kernels stay what they were.
#include "ring_rotate.hpp"

namespace tfhe_hip {

namespace {

template <int LOGN, bool ROWS>
__global__ __launch_bounds__(128) void ring_rotate_kernel(RingRotateArgs a) {
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t lds_scr[2][NTT::SCRATCH_WORDS];
    // residues in natural order, [prime = the wave that wrote them][output polynomial][N]
    __shared__ __align__(16) uint32_t lds_x[2][2][N];
    // the accumulator: torus words, [polynomial][N]
    __shared__ __align__(16) uint32_t lds_acc[2][N];
    __shared__ uint16_t lds_bar[ROTATE_MAX_LWE_N + 8];           // modulus-switched mask and body
    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const PrimeCtx c = ring_prime_ctx(q, a.tw, N);
    uint32_t *scr = lds_scr[q];

    const int wg = blockIdx.x;                                   // < a.count: the grid is a.count workgroups
    const int n = a.n;
    {
        const int32_t *lwe = a.lwe + (size_t)(a.lwe_index ? a.lwe_index[wg] : wg) * a.lwe_stride;
        // round(t 2N / 2^32) mod 2N (kernels.hip prelude_modswitch)
        for (int i = tid; i <= n; i += 128) lds_bar[i] = (uint16_t)(((uint32_t)lwe[i] + (1u << (30 - LOGN))) >> (31 - LOGN));
    }
    __syncthreads();
    {
        // ACC_0[q][j] = c[q][j + bbar] below N, -c[q][j + bbar - N] from N on, indices mod 2N (kernels.hip lut_coef)
        const int32_t *src = a.ring + ((size_t)(a.ring_index ? a.ring_index[wg] : wg) * 2 + q) * N;
        const int barb = lds_bar[n];
#pragma unroll
        for (int r = 0; r < REGS; ++r) {
            const int j = r * 64 + lane, idx = (j + barb) & (2 * N - 1);
            const uint32_t w = (uint32_t)src[idx & (N - 1)];
            lds_acc[q][j] = (idx & N) ? 0u - w : w;
        }
    }
    __syncthreads();

    const uint32_t mask = (1u << a.Bgbit) - 1u;
    const int32_t half = 1 << (a.Bgbit - 1);
    typename NTT::FwdTw0 t0;                 // lane-uniform and the same for every transform
    t0.load(c, lane);
    for (int i = 0; i < n; ++i) {
        const int abar = __builtin_amdgcn_readfirstlane((int)lds_bar[i]);
        if (abar == 0) continue;                                 // workgroup-uniform: both waves skip the step's barriers

        int64_t acc0[REGS], acc1[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) { acc0[r] = 0; acc1[r] = 0; }
        // image of row (i, u, p): [X = i (k+1) l + u l + p][prime][polynomial 2][N] (kernels.hip bk_transform_kernel, nw = 2)
        const uint4 *rowimg = reinterpret_cast<const uint4 *>(a.img + ((size_t)i * 2 * a.l * 2 + q) * 2 * N) + lane;
        for (int u = 0; u < 2; ++u) {
            // coefficient j = 64 r + lane of X^(abar) ACC[u] - ACC[u] (layout L0 of ntt_wave.hpp): (X^(abar) ACC)[j] =
            // ACC[j - abar], negated where (j - abar) mod 2N is N or more
            uint32_t v[REGS];
#pragma unroll
            for (int r = 0; r < REGS; ++r) {
                const int j = r * 64 + lane, idx = (j - abar) & (2 * N - 1);
                const uint32_t w = lds_acc[u][idx & (N - 1)];
                v[r] = ((idx & N) ? 0u - w : w) - lds_acc[u][j] + a.offset;
            }
            for (int p = 0; p < a.l; ++p) {
                const int shift = 32 - (p + 1) * a.Bgbit;
                int32_t x[REGS];
#pragma unroll
                for (int r = 0; r < REGS; ++r) x[r] = (int32_t)((v[r] >> shift) & mask) - half;    // |x| <= Bg/2 <= 2^11
                NTT::template forward<false>(x, c, scr, lane, t0);            // |x| < 6.1 P / 6.7 P (cmux.hpp)
                const uint4 *bp = rowimg + (size_t)(u * a.l + p) * N;       // 4N words per row = N uint4
#pragma unroll
                for (int g = 0; g < REGS / 4; ++g) {
                    const uint4 b0 = bp[g * 64], b1 = bp[N / 4 + g * 64];
                    acc0[4 * g + 0] += (int64_t)x[4 * g + 0] * (int32_t)b0.x;
                    acc0[4 * g + 1] += (int64_t)x[4 * g + 1] * (int32_t)b0.y;
                    acc0[4 * g + 2] += (int64_t)x[4 * g + 2] * (int32_t)b0.z;
                    acc0[4 * g + 3] += (int64_t)x[4 * g + 3] * (int32_t)b0.w;
                    acc1[4 * g + 0] += (int64_t)x[4 * g + 0] * (int32_t)b1.x;
                    acc1[4 * g + 1] += (int64_t)x[4 * g + 1] * (int32_t)b1.y;
                    acc1[4 * g + 2] += (int64_t)x[4 * g + 2] * (int32_t)b1.z;
                    acc1[4 * g + 3] += (int64_t)x[4 * g + 3] * (int32_t)b1.w;
                }
            }
        }
        // |acc| < (k+1) l f P^2 -> reduction below 4 P (MAC bound) -> inverse NTT: signed residues below P, natural order
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
        // the waves took different primes and now exchange through LDS alone (ntt_wave.hpp lds_barrier: both waves reach
        // it on the same path; nothing is stored to global memory inside the loop)
        lds_barrier();
        // wave q owns output polynomial q: coefficients 4 (64 g + lane) .. + 3, both primes' residues, the signed CRT
        // (the true integer is below CRT_EXACT_LIMIT: CRT bound), added to ACC[q] in place
        const uint4 *r0 = reinterpret_cast<const uint4 *>(lds_x[0][q]) + lane;
        const uint4 *r1 = reinterpret_cast<const uint4 *>(lds_x[1][q]) + lane;
        uint4 *dst = reinterpret_cast<uint4 *>(lds_acc[q]) + lane;
#pragma unroll
        for (int g = 0; g < REGS / 4; ++g) {
            const uint4 x0 = r0[g * 64], x1 = r1[g * 64], base = dst[g * 64];
            dst[g * 64] = make_uint4(base.x + crt_signed_to_torus((int32_t)x0.x, (int32_t)x1.x),
                                     base.y + crt_signed_to_torus((int32_t)x0.y, (int32_t)x1.y),
                                     base.z + crt_signed_to_torus((int32_t)x0.z, (int32_t)x1.z),
                                     base.w + crt_signed_to_torus((int32_t)x0.w, (int32_t)x1.w));
        }
        // the next step reads both polynomials of ACC and overwrites the residues
        lds_barrier();
    }

    if constexpr (!ROWS) {
        // wave q wrote ACC[q] itself, last: no barrier in front of its own read
        const uint4 *src = reinterpret_cast<const uint4 *>(lds_acc[q]) + lane;
        uint4 *dst = reinterpret_cast<uint4 *>(a.out + ((size_t)wg * 2 + q) * N) + lane;
#pragma unroll
        for (int g = 0; g < REGS / 4; ++g) dst[g * 64] = src[g * 64];
    } else {
        // (the loop's last barrier, or the prologue's, stands between the writes of ACC and these reads of both polynomials)
        const uint32_t *A = lds_acc[0], *B = lds_acc[1];
        constexpr int groups = N / 4;                            // mask groups; group `groups` is (b, 0, 0, 0)
        uint4 *row = reinterpret_cast<uint4 *>(a.rows.u_buf + (size_t)wg * a.rows.u_stride);
        for (int g = tid; g <= groups; g += 128) {
            uint4 w;
            if (g < groups) {
                // Extract_0: a_0 = A[0], a_i = -A[N - i]
                uint32_t m[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int d = 4 * g + t;
                    m[t] = d == 0 ? A[0] : 0u - A[N - d];
                }
                w = make_uint4(m[0], m[1], m[2], m[3]);
            } else {
                w = make_uint4(B[0], 0u, 0u, 0u);
            }
            row[g] = w;
        }
    }
}

}  // namespace

bool launch_ring_rotate(hipStream_t s, const RingRotateArgs &a) {
    // the kernel is instantiated for k = 1; everything it was bounded for is checked here once more
    if (ring_rotate_error(a)) return false;
    const dim3 grid(a.count), block(128);
    if (a.rows.u_buf) {
        if (a.N == 2048) hipLaunchKernelGGL((ring_rotate_kernel<11, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ring_rotate_kernel<10, true>), grid, block, 0, s, a);
    } else {
        if (a.N == 2048) hipLaunchKernelGGL((ring_rotate_kernel<11, false>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((ring_rotate_kernel<10, false>), grid, block, 0, s, a);
    }
    return true;
}

}  // namespace tfhe_hip
