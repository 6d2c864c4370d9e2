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
// kernels.hip and cmux.hip are not touched by this file; the few lines they keep private (the per-prime context) are
// restated here.
#include "ring_public.hpp"
#include "ntt_wave.hpp"

namespace tfhe_hip {

namespace {

// the twiddle tables of prime p (engine.cpp make_twiddles; the same lines as kernels.hip make_ctx)
__device__ __forceinline__ PrimeCtx public_ctx(int p, const uint32_t *tw, int n_ring) {
    PrimeCtx c;
    c.P = p ? NTT_P1 : NTT_P0;
    c.pinv = p ? NTT_PINV1 : NTT_PINV0;
    c.rmod = p ? NTT_R[1] : NTT_R[0];
    c.wf = tw + (size_t)(p * 2 + 0) * n_ring;
    c.wi = tw + (size_t)(p * 2 + 1) * n_ring;
    const uint4 *quads = reinterpret_cast<const uint4 *>(tw + (size_t)4 * n_ring);
    c.qf = quads + (size_t)(p * 2 + 0) * (n_ring / 2);
    c.qi = quads + (size_t)(p * 2 + 1) * (n_ring / 2);
    c.dtab = nullptr;
    c.fw1 = nullptr;
    c.fw2 = nullptr;
    return c;
}

// grid (count, 2 primes), one wave each
template <int LOGN>
__global__ __launch_bounds__(64) void public_image_kernel(PublicImageArgs a) {
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t scr[NTT::SCRATCH_WORDS];
    const int lane = threadIdx.x;
    const int p = blockIdx.y;
    const int poly = blockIdx.x;                                 // < a.count: the grid is a.count polynomials wide
    const PrimeCtx c = public_ctx(p, a.tw, N);
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
    const PrimeCtx c = public_ctx(p, a.tw, N);
    uint32_t *scr = lds_scr[p];
    const PublicRows &t = a.rows;

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
    // wave p owns output polynomial p: coefficients 4 (64 g + lane) .. + 3, both primes' residues, the signed CRT (the
    // true integer is below CRT_EXACT_LIMIT: CRT bound)
    const uint4 *r0 = reinterpret_cast<const uint4 *>(lds_x[0][p]) + lane;
    const uint4 *r1 = reinterpret_cast<const uint4 *>(lds_x[1][p]) + lane;
    // the torus words of polynomial p take the place of prime 0's residues: a lane writes the 16 bytes it alone read
    uint4 *tor = reinterpret_cast<uint4 *>(lds_x[0][p]) + lane;
    uint4 *full = a.out ? reinterpret_cast<uint4 *>(a.out + ((size_t)wg * 2 + p) * N) + lane : nullptr;    // uniform
#pragma unroll
    for (int g = 0; g < REGS / 4; ++g) {
        const uint4 x0 = r0[g * 64], x1 = r1[g * 64];
        const uint4 w = make_uint4(crt_signed_to_torus((int32_t)x0.x, (int32_t)x1.x), crt_signed_to_torus((int32_t)x0.y, (int32_t)x1.y),
                                   crt_signed_to_torus((int32_t)x0.z, (int32_t)x1.z), crt_signed_to_torus((int32_t)x0.w, (int32_t)x1.w));
        tor[g * 64] = w;
        if (full) full[g * 64] = w;
    }
    if (!t.u_buf) return;                                        // workgroup-uniform: the raw product form
    lds_barrier();
    // entry e of this product is row wg S + e of the launch: Extract_(e w) as ring_extract_kernel writes it, A and B in LDS
    const uint32_t *A = lds_x[0][0], *B = lds_x[0][1];
    const int S = N / t.width;
    const int rows = min(S, t.M - wg * S);                       // >= 1: the launcher checks (count - 1) S < M <= count S
    constexpr int groups = N / 4;                                // mask groups; group `groups` is (b, 0, 0, 0)
    for (int e = 0; e < rows; ++e) {
        const int ew = e * t.width;
        uint4 *row = reinterpret_cast<uint4 *>(t.u_buf + ((size_t)wg * S + e) * t.u_stride);
        for (int g = tid; g <= groups; g += 128) {
            uint4 w;
            if (g < groups) {
                uint32_t m[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int d = ew - (4 * g + i);
                    m[i] = d >= 0 ? A[d] : 0u - A[d + N];
                }
                w = make_uint4(m[0], m[1], m[2], m[3]);
            } else {
                w = make_uint4(B[ew], 0u, 0u, 0u);
            }
            row[g] = w;
        }
    }
}

}  // namespace

bool launch_public_image(hipStream_t s, const PublicImageArgs &a) {
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > PUBLIC_MAX_POLYS || !a.polys || !a.img || !a.tw ||
        (reinterpret_cast<uintptr_t>(a.img) & 15u))
        return false;
    if (a.N == 2048) hipLaunchKernelGGL((public_image_kernel<11>), dim3(a.count, 2), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((public_image_kernel<10>), dim3(a.count, 2), dim3(64), 0, s, a);
    return true;
}

bool launch_public(hipStream_t s, const PublicArgs &a) {
    const PublicRows &t = a.rows;
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > PUBLIC_MAX_COUNT || (a.img_step != 0 && a.img_step != 1) ||
        (a.ring_stride != 0 && (a.ring_stride < 2 * (int64_t)a.N || (a.ring_stride & 3))) || !a.ring || !a.img || !a.tw ||
        (!a.out && !t.u_buf) || ((reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.img)) & 15u))
        return false;
    if (t.u_buf) {
        // rows: w a power of two in 1 .. N, every workgroup has an entry ((count - 1) S < M <= count S), one chunk at most
        if (t.width < 1 || t.width > a.N || (t.width & (t.width - 1)) || t.u_stride != a.N + 4 || (reinterpret_cast<uintptr_t>(t.u_buf) & 15u))
            return false;
        const int64_t S = a.N / t.width;
        if (t.M < 1 || t.M > UNPACK_CHUNK || t.M > a.count * S || t.M <= (a.count - 1) * S) return false;
    }
    if (a.N == 2048) hipLaunchKernelGGL((public_kernel<11>), dim3(a.count), dim3(128), 0, s, a);
    else hipLaunchKernelGGL((public_kernel<10>), dim3(a.count), dim3(128), 0, s, a);
    return true;
}

}  // namespace tfhe_hip
