// cmux.hpp -- the leveled half of TFHE (include/tfhe_hip.h "private selection"): the external product of a TGSW sample
// with a ring sample, G (.) c, the CMUX built from it, and the tree of CMUXes that selects one of M resident ring samples
// under d encrypted index bits.  Host-visible side of cmux.hip: the two magnitude bounds the kernel rests on, as checked
// functions, and the launcher.  Shared by the selector's constructor (select_host.cpp: a gadget the bounds cannot take is
// refused there), the engine and the kernel (static_asserts next to it).
//
// What the kernel computes for one CMUX under the rows G.row(u, p), u <= k = 1, p < l, of one selector bit:
//     diff     = d1 - d0                                        word-wise, wrapping
//     dig[u][p] = ((diff[u] + offset) >> (32 - (p+1) Bgbit) & (Bg - 1)) - Bg/2     signed digits in [-Bg/2, Bg/2)
//     out[w]   = d0[w] + sum_{u, p} dig[u][p](X) * G.row(u, p)[w](X)               in Z[X]/(X^N + 1), mod 2^32
// with the row words taken as signed 32-bit integers, through the two-prime NTT of ntt_wave.hpp: (k+1) l forward
// transforms, a 64-bit multiply-accumulate against the rows' NTT image (the bootstrapping-key image of kernels.hip
// bk_transform_kernel, n = the number of selector bits), ONE Montgomery reduction and inverse transform per prime and
// output polynomial, the signed CRT.  Two bounds make that exact; both are derived here and neither is tuned.
//
// Forward input bound relied on.  The digits are SIGNED here (pack's are unsigned and below 16): |dig| <= Bg/2 <= 2^11,
// since Bgbit <= 12.  That is the bound ntt_wave.hpp states for WaveNtt::forward on gadget digits -- "|x| <= 2^11 ends
// below 6.1 P (N = 1024) / 6.7 P (N = 2048)" -- and pack_forward_bound (pack.hpp: the recurrence of the pass structure,
// which takes magnitudes and so holds for either sign) run from 2^11 confirms it: cmux_forward_bound below.
//
// MAC bound (how many products one int64 accumulator takes before its reduction).
//   rows = (k+1) l products of a transform output |x| < f P (f = cmux_forward_bound) and a canonical image word
//   0 <= w < P: |acc| < rows f P^2; its Montgomery reduction is below rows f P^2 / 2^32 + P/2, and the inverse transform
//   takes inputs below 4 P (make_inv_plan), hence
//       rows * f * P / 2^32 < 3.5            rows <= 18, l <= 9 (N = 1024);   rows <= 16, l <= 8 (N = 2048)
//   (|acc| < 3.5 P 2^32 < 2^61 then holds with it: no int64 overflow).  This is the inequality of the 2-wave blind
//   rotation (br_forms.hpp BR_FORM_WAVE2), the widest of the forms, restated for this kernel's single reduction: every
//   gadget a cloud key is accepted with passes it (tests/test_select_cpu.py enumerates them).
// CRT bound (the true integer of an output coefficient must be what the signed CRT returns).
//   A coefficient of sum dig * row is a sum of rows * N products of a digit and a row word:
//       |S| <= (k+1) l * N * (Bg/2) * 2^31 < CRT_EXACT_LIMIT
//   (ntt_field.hpp: 0.36 P0 P1, the limit the signed lazy residues need) -- the bound unsupported_reason (engine.cpp)
//   applies to a cloud key, for the same sum.  All digits at -Bg/2 against rows of 0x80000000 reach the left side exactly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntt_field.hpp"
#include "pack.hpp"
#include "ring_wave.hpp"

namespace tfhe_hip {

constexpr int CMUX_MAX_BGBIT = 12;
// the most index bits a selector may carry: 2^20 resident ring samples are 8 GB at N = 1024
constexpr int SELECT_MAX_BITS = 20;

// |outputs| / P of a forward transform of WaveNtt<logn> on signed gadget digits, |x| <= 2^11
constexpr double cmux_forward_bound(int logn) { return pack_forward_bound(logn, (double)(1 << (CMUX_MAX_BGBIT - 1))); }
// MAC bound: `rows` = (k+1) l products into one accumulator, then the reduction, must leave the inverse transform inputs below 4 P
constexpr bool cmux_mac_ok(int N, int rows) {
    const double P = (double)NTT_P[1];
    return rows >= 1 && (double)rows * cmux_forward_bound(pack_logn(N)) * P / 4294967296.0 < 3.5;
}
// CRT bound: rows N (Bg/2) 2^31 < CRT_EXACT_LIMIT
constexpr bool cmux_crt_ok(int N, int rows, int Bgbit) {
    // a 2^31 < L  <=>  a <= (L - 1) >> 31, which keeps the comparison inside 64 bits
    return rows >= 1 && Bgbit >= 1 && Bgbit <= CMUX_MAX_BGBIT &&
           (uint64_t)rows * (uint64_t)N * (uint64_t)(1u << (Bgbit - 1)) <= ((CRT_EXACT_LIMIT - 1) >> 31);
}
static_assert(cmux_forward_bound(10) < 6.1 && cmux_forward_bound(11) < 6.7, "forward bounds of ntt_wave.hpp for digits up to 2^11");
static_assert(cmux_mac_ok(1024, 18) && !cmux_mac_ok(1024, 19) && cmux_mac_ok(2048, 16) && !cmux_mac_ok(2048, 17), "MAC bound");
static_assert(cmux_crt_ok(1024, 6, 7) && cmux_crt_ok(1024, 4, 10) && !cmux_crt_ok(1024, 6, 10) && cmux_crt_ok(2048, 6, 6),
              "CRT bound: the built-in sets hold, l = 3 at Bgbit = 10 does not");

// null if the kernel runs gadget (l, Bgbit) of ring (N, k) exactly, else what is wrong with it
inline const char *cmux_gadget_error(int N, int k, int l, int Bgbit) {
    if ((N != 1024 && N != 2048) || k != 1) return "the CMUX kernel is built for N = 1024 or 2048 and k = 1";
    if (l < 1 || Bgbit < 1 || Bgbit > CMUX_MAX_BGBIT || l * Bgbit > 32) return "gadget digits must fit 12 bits and l * Bgbit <= 32";
    if (!cmux_mac_ok(N, (k + 1) * l))
        return "(k+1) l gadget rows exceed what one 64-bit accumulator takes before its reduction (cmux.hpp MAC bound)";
    if (!cmux_crt_ok(N, (k + 1) * l, Bgbit))
        return "the gadget exceeds the exact range of the two-prime CRT (cmux.hpp CRT bound)";
    return nullptr;
}

// One launch: `count` independent CMUXes under selector bit `bit`.  CMUX c reads d0 at d0[c * stride] and d1 at
// d1[c * stride] (2N words each: the mask polynomial, then the body) and writes out[c * 2N]; from c = n_d1 on d1 is the
// all-zero sample and is not read (a tree level whose last pair has no right entry).  A tree level over entries e[0..cnt)
// is d0 = e, d1 = e + 2N, stride = 4N, count = ceil(cnt / 2), n_d1 = cnt / 2.  out overlaps neither input.
// img: the rows' NTT image (launch_bk_transform of the selector's words [nbits][(k+1) l][2][N] with nw = 2).
// rot != 0 (0 < rot < N): a launch of rotation steps of the packed lookup (include/tfhe_hip.h), CMUX c being
// ROT(G, rot, d0[c]) = CMUX(G, X^(-rot) d0[c], d0[c]) with (X^(-rot) c)[u][j] = c[u][j + rot] for j + rot < N and
// -c[u][j + rot - N] otherwise; d1 and n_d1 are not read, and out must not overlap d0 (the launcher refuses it).
struct CmuxArgs {
    int32_t N, l, Bgbit, bit, count, n_d1;
    int64_t stride;
    uint32_t offset;                // sum_p (Bg/2) 2^(32 - p Bgbit): the decomposition's offset
    int32_t rot;                    // 0: a CMUX of (d1, d0); else the rotation step's monomial power (in what was padding)
    const int32_t *d0, *d1;
    const uint32_t *img;
    const uint32_t *tw;             // the twiddle tables of the ring (engine.cpp make_twiddles)
    int32_t *out;
};
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_cmux(hipStream_t s, const CmuxArgs &a);

// The product alone, G (.) c, with a fused sample extraction (include/tfhe_hip.h "encrypted inner products").  G may be the
// TGSW sample of a small-integer POLYNOMIAL: only the row words differ from those of a bit, and both bounds above take the
// row words as arbitrary 32-bit words -- the MAC bound through the canonical image word below P, the CRT bound through
// |word| <= 2^31 -- so they hold unchanged and there is no third bound.  The operand is c itself (the digits of c + offset),
// nothing is added to the sum.
// One launch: c.count workgroups, workgroup r on the ring sample at c.d0[r * c.stride] under selector sample c.bit.
// rows.u_buf != null: the rows Extract_(e width)(G (.) c_r) of ring_wave.hpp RingRows, passing ring_rows_error.  c.out !=
// null: the full products out[r * 2N] as well (the raw test form; alone when u_buf is null).  c.d1, c.n_d1 and c.rot are
// not used and must be zero.
struct InnerArgs {
    CmuxArgs c;
    RingRows rows;
};
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_inner(hipStream_t s, const InnerArgs &a);

}  // namespace tfhe_hip
