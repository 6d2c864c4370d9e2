// ring_inner_sum.hpp -- sums of TGSW products over several ring samples (include/tfhe_hip.h "TGSW products over several
// ring samples"): the TGSW counterpart of ring_public.hpp's summed public product, for galleries that rest ENCRYPTED.
// Host-visible side of ring_inner_sum.hip: the two bounds the kernel rests on, as checked functions, and the launcher.
// Shared by the host entries (inner_sum_host.cpp), the engine and the kernel.
//
// What the kernel computes for one group g of K = terms ring samples c_(gK) .. c_(gK+K-1) under the K consecutive selector
// samples G_b .. G_(b+K-1), exactly in Z[X]/(X^N + 1) mod 2^32:
//     out[g] = sum_(t < K) G_(b+t) (.) c_(gK+t)
// with G (.) c as cmux.hpp defines it (the offset decomposition of c, signed digits in [-Bg/2, Bg/2), the row words taken as
// signed 32-bit integers).  Per prime: K (k+1) l forward transforms, their products with the rows' image words added into
// the SAME two 64-bit accumulators, ONE inverse transform per output polynomial, the signed CRT once.  K = 1 computes
// inner_kernel's words.  The forward input bound is cmux.hpp's (|dig| <= 2^11, outputs below f P, f = cmux_forward_bound:
// 6.1 / 6.7).  The other two bounds change; both are derived here and neither is tuned.
//
// MAC bound: the accumulator is FOLDED between blocks of rows.
//   cmux.hpp: one accumulator takes `rows` products with rows f P / 2^32 < 3.5 before its one reduction -- 18 rows
//   (N = 1024), 16 (N = 2048) --, and a term of a built-in gadget has (k+1) l = 6 of them: three terms, or two, and no more.
//   So after every B rows the accumulator is folded in place:
//       y = mont_redc(acc)         y = acc 2^-32 mod P,  |y| < |acc| / 2^32 + P/2          (ntt_wave.hpp)
//       acc = (int64) y * R        R = 2^32 mod P (NTT_R, PrimeCtx::rmod): acc is again the same residue mod P
//   Only the residue of the accumulator enters the result (the last reduction, the inverse transform and the CRT read
//   nothing else), so the partial blocks combine exactly.  Magnitudes: a block of B rows on top of a fold is below
//   B f P^2 + |y| R, and with the block's own reduction below 4 P -- which is what is to be shown -- |y| < 4 P, so the fold
//   re-enters as 4 R / P in units of P^2: R = 3,407,840 (prime 0), 1,310,688 (prime 1), at most 0.0255 P, so 0.102 against
//   a row's f = 6.1: a sixtieth of one row.  The inequality of a block, the first one (no fold under it) a fortiori:
//       (B f + 4 R / P) P / 2^32 < 3.5         B = 18 rows (N = 1024),  B = 16 rows (N = 2048)
//   -- the block lengths cmux.hpp found for one reduction: the fold costs no row.  Then every reduction, the last one
//   included, is below 3.5 P + P/2 = 4 P, the inverse transform's input bound (make_inv_plan), and |acc| < 3.5 P 2^32 <
//   2^61: no int64 overflow.  Induction over the blocks: the first fold's |y| < 4 P by cmux.hpp's bound, every later one by
//   this inequality.  A block boundary may fall INSIDE a term (B counts rows, not terms: l = 4 has 8 rows a term).
//   The MAC side therefore sets no limit on K.
// CRT bound (the true integer of an output coefficient must be what the signed CRT returns).
//   A coefficient of the sum is a sum of K (k+1) l N products of a digit and a row word:
//       |S| <= K (k+1) l N (Bg/2) 2^31 < CRT_EXACT_LIMIT
//   cmux.hpp's bound with K (k+1) l rows.  Built-in gadgets, (l, Bgbit) = (3, 7) at N = 1024 and (3, 6) at N = 2048:
//   K 2^49.58 < 2^52.5 holds up to K = 7.  All digits at -Bg/2 against rows of 0x80000000 reach the left side exactly.
// INNER_SUM_MAX_TERMS = 8 caps K (the public sum's cap); inner_sum_max_terms is the largest K <= 8 the CRT bound takes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmux.hpp"

namespace tfhe_hip {

constexpr int INNER_SUM_MAX_TERMS = 8;
// the most groups one raw launch takes
constexpr int32_t INNER_SUM_MAX_GROUPS = 1 << 16;

// what a fold adds to the next block, in units of P^2: |y| R < 4 P R, the larger R over the smaller P
constexpr double inner_sum_fold_bound() {
    const double R = (double)(NTT_R[0] > NTT_R[1] ? NTT_R[0] : NTT_R[1]), P = (double)(NTT_P[0] < NTT_P[1] ? NTT_P[0] : NTT_P[1]);
    return 4.0 * R / P;
}
// MAC bound of one block: `rows` products on top of a folded accumulator, then the reduction, below 4 P
constexpr bool inner_sum_block_ok(int N, int rows) {
    const double P = (double)NTT_P[1];
    return rows >= 1 && ((double)rows * cmux_forward_bound(pack_logn(N)) + inner_sum_fold_bound()) * P / 4294967296.0 < 3.5;
}
// the block length: the most rows between two folds
constexpr int inner_sum_block_rows(int N) {
    int B = 0;
    while (B < 64 && inner_sum_block_ok(N, B + 1)) ++B;
    return B;
}
// CRT bound: terms (k+1) l N (Bg/2) 2^31 < CRT_EXACT_LIMIT
constexpr bool inner_sum_crt_ok(int N, int l, int Bgbit, int terms) {
    return terms >= 1 && l >= 1 && cmux_crt_ok(N, terms * 2 * l, Bgbit);
}
// the largest K in 1 .. INNER_SUM_MAX_TERMS both bounds take for gadget (l, Bgbit); 0 if not even one term passes
constexpr int inner_sum_max_terms(int N, int l, int Bgbit) {
    int K = 0;
    while (K < INNER_SUM_MAX_TERMS && inner_sum_block_rows(N) >= 1 && inner_sum_crt_ok(N, l, Bgbit, K + 1)) ++K;
    return K;
}
static_assert(inner_sum_fold_bound() < 0.102, "the fold re-enters below 0.102 P^2, a sixtieth of a row");
static_assert(inner_sum_block_rows(1024) == 18 && inner_sum_block_rows(2048) == 16, "block lengths: the fold costs no row of cmux.hpp's 18 and 16");
static_assert(cmux_mac_ok(1024, inner_sum_block_rows(1024)) && cmux_mac_ok(2048, inner_sum_block_rows(2048)),
              "the first block, with no fold under it, is cmux.hpp's MAC bound");
static_assert((18.0 * cmux_forward_bound(10) + inner_sum_fold_bound()) * (double)NTT_P[1] * (double)NTT_P[1] < 2305843009213693952.0 &&
                  (16.0 * cmux_forward_bound(11) + inner_sum_fold_bound()) * (double)NTT_P[1] * (double)NTT_P[1] < 2305843009213693952.0,
              "the accumulator stays below 2^61");
static_assert(inner_sum_max_terms(1024, 3, 7) == 7 && inner_sum_max_terms(2048, 3, 6) == 7 && !inner_sum_crt_ok(1024, 3, 7, 8) &&
                  !inner_sum_crt_ok(2048, 3, 6, 8),
              "CRT bound: K <= 7 at the built-in gadgets");
static_assert(inner_sum_max_terms(1024, 4, 5) == INNER_SUM_MAX_TERMS && inner_sum_max_terms(1024, 2, 10) == 1 && inner_sum_max_terms(1024, 3, 10) == 0,
              "the cap where the CRT bound is far, one term at the legacy gadget, none where cmux.hpp refuses the gadget");

// One launch of c.count workgroups: workgroup g forms sum_(t < terms) G_(c.bit + t) (.) c_t from the `terms` ring samples at
// c.d0[g * c.stride + t * 2N] (c.stride >= terms 2N) under the selector samples c.bit .. c.bit + terms - 1 of image c.img.
// block: inner_sum_block_rows(c.N), the rows between two folds (the launcher refuses any other value).
// rows / c.out: as InnerArgs, entry e of workgroup g being row g S + e.  c.d1, c.n_d1 and c.rot are not used and must be zero.
struct InnerSumArgs {
    CmuxArgs c;
    int32_t terms, block;
    RingRows rows;
};
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_inner_sum(hipStream_t s, const InnerSumArgs &a);

}  // namespace tfhe_hip
