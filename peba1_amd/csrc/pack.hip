// pack.hip -- the packing key switch on gfx950 (pack.hpp has the definition of a chunk and the two bounds).
//
//   pack_kernel          one workgroup of two wave64 per range of mask indices; wave q works modulo prime q.  Per mask
//                        index i (one chunk): each lane gathers word i of its samples' rows once (coefficient j of every
//                        digit polynomial comes from sample j: 16 or 32 strided words per lane, zeros from `count` on),
//                        then for each of the t digits one forward NTT of the digit polynomial and a 64-bit
//                        multiply-accumulate against the two polynomials of the key row's image; after the t rows one
//                        Montgomery reduction and inverse NTT per polynomial, the residues of one polynomial handed to
//                        the partner wave through LDS, the signed CRT, and the sum added to a register-resident Torus32
//                        partial of the polynomial the wave owns (wave q owns polynomial q).  Partials go to scratch.
//   pack_reduce_kernel   sums the partials, negates, adds sum_j b_j X^j to the body: the 2N words of the result.
// No atomics; the result does not depend on the order anything ran in.
//
// kernels.hip is not touched by this file; the few lines it keeps private (the per-prime context) are restated once, in
// ring_wave.hpp.
#include "pack.hpp"
#include "ring_wave.hpp"

namespace tfhe_hip {

namespace {

// the largest t any accepted decomposition has: the accumulators below take that many products (pack.hpp MAC bound)
static_assert(pack_mac_ok(1024, 18) && pack_mac_ok(2048, 16), "rows one accumulator takes");

template <int LOGN>
__global__ __launch_bounds__(128) void pack_kernel(PackArgs a) {
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t lds_scr[2][NTT::SCRATCH_WORDS];
    // residues on their way to the partner wave: [parity of the chunk][sending wave][N].  Two parities, one barrier per
    // chunk: a wave writes parity b again only two chunks later, i.e. after a barrier its partner reached having read b.
    __shared__ uint32_t lds_x[2][2][N];
    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const PrimeCtx c = ring_prime_ctx(q, a.tw, N);
    uint32_t *scr = lds_scr[q];

    // coefficient j = 64 r + lane of every digit polynomial comes from sample j (layout L0 of ntt_wave.hpp)
    int32_t row_of[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) {
        const int j = r * 64 + lane;
        row_of[r] = j < a.count ? (a.slots ? a.slots[j] : j) : -1;
    }
    const uint32_t prec = pack_prec_offset(a.t, a.basebit);
    const uint32_t mask = (1u << a.basebit) - 1u;
    const int i0 = blockIdx.x * a.idx_per_wg;
    const int i1 = min(a.n, i0 + a.idx_per_wg);
    typename NTT::FwdTw0 t0;                 // lane-uniform and the same for every transform
    t0.load(c, lane);

    uint32_t part[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) part[r] = 0u;

    for (int i = i0; i < i1; ++i) {
        uint32_t v[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r)
            v[r] = row_of[r] >= 0 ? (uint32_t)a.samples[(size_t)row_of[r] * a.stride + i] + prec : 0u;
        int64_t acc0[REGS], acc1[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) { acc0[r] = 0; acc1[r] = 0; }
        // image of row (i, p): [X = i t + p][prime][polynomial 2][N] (kernels.hip bk_transform_kernel, nw = 2)
        const uint4 *rowimg = reinterpret_cast<const uint4 *>(a.img + ((size_t)i * a.t * 2 + q) * 2 * N) + lane;
        for (int p = 0; p < a.t; ++p) {
            const int shift = 32 - (p + 1) * a.basebit;
            int32_t x[REGS];
#pragma unroll
            for (int r = 0; r < REGS; ++r) x[r] = (int32_t)((v[r] >> shift) & mask);
            NTT::template forward<false>(x, c, scr, lane, t0);            // |x| < 6.1 P / 6.7 P (pack.hpp)
            const uint4 *bp = rowimg + (size_t)p * N;                   // 4N words per row = N uint4
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
        // |acc| < t f P^2 -> reduction below 4 P (MAC bound) -> inverse NTT: signed residues below P, natural order
        int32_t y0[REGS], y1[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) y0[r] = mont_redc(acc0[r], c.P, c.pinv);
        NTT::inverse(y0, c, scr, lane);
#pragma unroll
        for (int r = 0; r < REGS; ++r) y1[r] = mont_redc(acc1[r], c.P, c.pinv);
        NTT::inverse(y1, c, scr, lane);
        // wave q keeps polynomial q and hands its residues of the other one over
        const int par = (i - i0) & 1;
        uint32_t *xs = lds_x[par][q];
#pragma unroll
        for (int r = 0; r < REGS; ++r) xs[r * 64 + lane] = (uint32_t)(q ? y0[r] : y1[r]);
        __syncthreads();
        const uint32_t *xr = lds_x[par][1 - q];
#pragma unroll
        for (int r = 0; r < REGS; ++r) {
            const int32_t other = (int32_t)xr[r * 64 + lane];
            // the chunk's true integer is below CRT_EXACT_LIMIT (CRT bound): its low 32 bits, summed mod 2^32
            part[r] += q ? crt_signed_to_torus(other, y1[r]) : crt_signed_to_torus(y0[r], other);
        }
    }
    int32_t *dst = a.partial + ((size_t)blockIdx.x * 2 + q) * N;
#pragma unroll
    for (int r = 0; r < REGS; ++r) dst[r * 64 + lane] = (int32_t)part[r];
}

// out[w] = (w in the body and w - N < count ? b_{w - N} : 0) - sum_g partial[g][w]; a block of four waves per 64 words
__global__ __launch_bounds__(256) void pack_reduce_kernel(PackArgs a, int groups) {
    __shared__ uint32_t red[4][64];
    const int lane = threadIdx.x & 63, piece = threadIdx.x >> 6;
    const int w = blockIdx.x * 64 + lane;                 // < 2N: the grid is 2N / 64 blocks
    const size_t words = (size_t)2 * a.N;
    uint32_t s = 0;
    for (int g = piece; g < groups; g += 4) s += (uint32_t)a.partial[(size_t)g * words + w];
    red[piece][lane] = s;
    __syncthreads();
    if (piece == 0) {
        const uint32_t total = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
        uint32_t body = 0;
        const int j = w - a.N;
        if (j >= 0 && j < a.count) body = (uint32_t)a.samples[(size_t)(a.slots ? a.slots[j] : j) * a.stride + a.n];
        a.out[w] = (int32_t)(body - total);
    }
}

}  // namespace

bool launch_pack(hipStream_t s, const PackArgs &a) {
    // the kernel is instantiated for k = 1; everything else it was bounded for is checked here once more
    if (pack_decomp_error(a.N, 1, a.t, a.basebit) || a.n < 1 || a.count < 1 || a.count > a.N || a.idx_per_wg < 1 ||
        a.stride <= a.n || !a.samples || !a.img || !a.tw || !a.partial || !a.out)
        return false;
    const int groups = pack_groups(a.n, a.idx_per_wg);
    if (a.N == 2048) hipLaunchKernelGGL(pack_kernel<11>, dim3(groups), dim3(128), 0, s, a);
    else hipLaunchKernelGGL(pack_kernel<10>, dim3(groups), dim3(128), 0, s, a);
    hipLaunchKernelGGL(pack_reduce_kernel, dim3(2 * a.N / 64), dim3(256), 0, s, a, groups);
    return true;
}

}  // namespace tfhe_hip
