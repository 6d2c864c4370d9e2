// ring_wave.hpp -- what the two-wave ring kernels outside kernels.hip share (pack.hip, cmux.hip, ring_public.hip): the rows
// a launch leaves for the key switch with their launcher check, and on the device pass the per-prime context and the
// CRT-and-rows tail.  kernels.hip does not include this file: its make_ctx and ring_prime_ctx below are the two statements
// of the twiddle layout that remain.
#pragma once
#include <stdint.h>

#include "unpack.hpp"

namespace tfhe_hip {

// The rows of one launch (cmux.hpp InnerArgs, ring_public.hpp PublicArgs).  u_buf != null: workgroup g's product holds
// S = N / width entries and entry e < S is written as row g S + e of u_buf,
//     Extract_(e width)(A, B):  a_i = A[e w - i] for i <= e w,  a_i = -A[N + e w - i] past it,  b = B[e w],
// in the layout of ring_extract_kernel (unpack.hpp: u_stride = N + 4 words a row, the body and three zeros last, 16-byte
// aligned), for the rows below M alone.
struct RingRows {
    int32_t M = 0, width = 1, u_stride = 0;
    int32_t *u_buf = nullptr;
};

// null if `count` workgroups of ring N write M rows of entries `width` apart, else what is wrong: w a power of two in
// 1 .. N, every workgroup has an entry ((count - 1) S < M <= count S), one chunk at most
constexpr const char *ring_rows_error(int N, int count, int M, int width, int u_stride) {
    if (width < 1 || width > N || (width & (width - 1))) return "width must be a power of two in 1..N";
    if (u_stride != N + 4) return "a row is N + 4 words";
    const int64_t S = N / width;
    if (M < 1 || M > UNPACK_CHUNK) return "a launch writes 1..UNPACK_CHUNK rows";
    if (M > count * S || M <= (count - 1) * S) return "every workgroup needs a row: (count - 1) S < M <= count S";
    return nullptr;
}
constexpr bool ring_rows_edges_ok(int N) {
    const int S = N / 4, full = UNPACK_CHUNK / N;     // three workgroups at width 4; `full` workgroups of S = N fill a chunk
    return !ring_rows_error(N, 3, 3 * S, 4, N + 4) && ring_rows_error(N, 3, 2 * S, 4, N + 4) && !ring_rows_error(N, 3, 2 * S + 1, 4, N + 4) &&
           !ring_rows_error(N, 5, 5, N, N + 4) && !ring_rows_error(N, 2, N + 1, 1, N + 4) && ring_rows_error(N, 3, 3, 3, N + 4) &&
           ring_rows_error(N, 1, 1, 2 * N, N + 4) && !ring_rows_error(N, full, UNPACK_CHUNK, 1, N + 4) &&
           ring_rows_error(N, full + 1, UNPACK_CHUNK + 1, 1, N + 4) && ring_rows_error(N, 3, 3 * S, 4, N);
}
static_assert(ring_rows_edges_ok(1024) && ring_rows_edges_ok(2048),
              "M = count S, (count - 1) S + 1, S = 1, S = N hold; (count - 1) S, width 3, 2 N, a second chunk, u_stride N do not");

// ntt_wave.hpp make_inv_plan(logn) in plain words, for the host's compiler, which cannot read that file: the inverse
// transform's steps, their fan (4 or 2), which of them renormalise, the bound of its outputs in units of the larger prime
// (include/tfhe_hip.h tfhe_hip_test_ntt_bounds; defined in ring_public.hip, beside the kernels that run the plan).
struct InvPlanWords {
    int32_t nsteps;
    int32_t fan[12], renorm[12];
    double out_bound;
};
InvPlanWords inv_plan_words(int logn);

}  // namespace tfhe_hip

// the device half: ntt_wave.hpp is device code, and the host's compiler reads this file through cmux.hpp and ring_public.hpp
#ifdef __HIPCC__
#include "ntt_wave.hpp"

namespace tfhe_hip {

// The twiddle tables of one prime.  engine.cpp make_twiddles owns the layout: four radix-2 tables [prime][forward,
// inverse][N], then the radix-4 quads at word 4 N in the same order, N / 2 entries each.
__device__ __forceinline__ PrimeCtx ring_prime_ctx(int prime, const uint32_t *tw, int n_ring) {
    PrimeCtx c;
    c.P = prime ? NTT_P1 : NTT_P0;
    c.pinv = prime ? NTT_PINV1 : NTT_PINV0;
    c.rmod = prime ? NTT_R[1] : NTT_R[0];
    c.wf = tw + (size_t)(prime * 2 + 0) * n_ring;
    c.wi = tw + (size_t)(prime * 2 + 1) * n_ring;
    const uint4 *quads = reinterpret_cast<const uint4 *>(tw + (size_t)4 * n_ring);
    c.qf = quads + (size_t)(prime * 2 + 0) * (n_ring / 2);
    c.qi = quads + (size_t)(prime * 2 + 1) * (n_ring / 2);
    c.dtab = nullptr;
    c.fw1 = nullptr;
    c.fw2 = nullptr;
    return c;
}

// The tail of a product kernel.  lds_x holds the residues in natural order, [prime = the wave that wrote them][output
// polynomial][N], and the caller has passed its lds_barrier() after the inverse transforms.  Wave `prime` owns output
// polynomial `prime`: it reads four consecutive coefficients 4 (64 g + lane) .. + 3 of both primes and applies the signed
// CRT (the true integer is below CRT_EXACT_LIMIT: the caller's CRT bound).  The torus words take the place of prime 0's
// residues -- a lane writes the 16 bytes it alone read -- and go to full_out[(wg 2 + prime) N] as well where full_out is
// not null (workgroup-uniform).  t.u_buf == null: the raw product form, nothing more.  Else one more barrier, and the two
// waves write the rows of workgroup wg (RingRows above) from A and B in LDS: a lane owns 16-byte groups of a row and reads
// the mask polynomial descending from A[e w - 4 g], negated past the wrap; the last group is (B[e w], 0, 0, 0).
template <int LOGN>
__device__ __forceinline__ void ring_crt_rows(uint32_t (&lds_x)[2][2][WaveNtt<LOGN>::N], int prime, int lane, int tid, int wg,
                                              int32_t *full_out, const RingRows &t) {
    constexpr int N = WaveNtt<LOGN>::N, REGS = WaveNtt<LOGN>::REGS;
    const uint4 *r0 = reinterpret_cast<const uint4 *>(lds_x[0][prime]) + lane;
    const uint4 *r1 = reinterpret_cast<const uint4 *>(lds_x[1][prime]) + lane;
    uint4 *tor = reinterpret_cast<uint4 *>(lds_x[0][prime]) + lane;
    uint4 *full = full_out ? reinterpret_cast<uint4 *>(full_out + ((size_t)wg * 2 + prime) * N) + lane : nullptr;
#pragma unroll
    for (int g = 0; g < REGS / 4; ++g) {
        const uint4 x0 = r0[g * 64], x1 = r1[g * 64];
        const uint4 w = make_uint4(crt_signed_to_torus((int32_t)x0.x, (int32_t)x1.x), crt_signed_to_torus((int32_t)x0.y, (int32_t)x1.y),
                                   crt_signed_to_torus((int32_t)x0.z, (int32_t)x1.z), crt_signed_to_torus((int32_t)x0.w, (int32_t)x1.w));
        tor[g * 64] = w;
        if (full) full[g * 64] = w;
    }
    if (!t.u_buf) return;                                        // workgroup-uniform
    lds_barrier();
    const uint32_t *A = lds_x[0][0], *B = lds_x[0][1];
    const int S = N / t.width;
    const int rows = min(S, t.M - wg * S);                       // >= 1: ring_rows_error, (count - 1) S < M <= count S
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

}  // namespace tfhe_hip
#endif
