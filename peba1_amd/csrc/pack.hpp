// pack.hpp -- the packing key switch (include/tfhe_hip.h "packing key switch"): up to N LWE samples under the LWE key
// become ONE TLWE sample under the ring key.  Host-visible side of pack.hip: the two magnitude bounds the kernel rests
// on, as checked functions, and the launcher.  Shared by the key constructors (shim.cpp / pack_host.cpp: a decomposition
// the bounds cannot take is refused there), the engine and the kernel (static_asserts next to it).
//
// What the kernel computes for one mask index i -- its CHUNK, `rows` = t rows of the key:
//     S_i(X) = sum_{p < t} D[i][p](X) * row[i][p](X)        in Z[X]/(X^N + 1), per polynomial of the row
// with digit polynomials 0 <= D < base = 2^basebit and key words taken as signed 32-bit integers, through the two-prime
// NTT of ntt_wave.hpp: t forward transforms, a 64-bit multiply-accumulate against the key's NTT image, ONE Montgomery
// reduction and inverse transform per prime and polynomial, the signed CRT.  The chunks' low 32 bits are then summed
// mod 2^32.  Two bounds make that exact; both are derived here and neither is tuned.
//
// MAC bound (how many products one int64 accumulator takes before its reduction).
//   A forward transform of digits grows a value by at most P + 3|x| P / 2^32 per radix-4 step (|A| <= |x2| P / 2^32 + P/2,
//   |S| <= (|x1| + |x3|) P / 2^32 + P/2: ntt_wave.hpp) and by P/2 + |x| P / 2^32 per radix-2 stage; pack_forward_bound
//   runs that recurrence over the pass structure of WaveNtt<LOGN> from |x| <= 15 (basebit <= 4): the outputs stay below
//   6.04 P (N = 1024) / 6.63 P (N = 2048) -- inside the 6.1 P / 6.7 P that ntt_wave.hpp states for digits below 2^11.
//   A word of the key image is canonical, 0 <= w < P.  So after `rows` products |acc| < rows * f * P^2 (f = that factor),
//   and its Montgomery reduction is below rows * f * P^2 / 2^32 + P/2.  The inverse transform takes inputs below 4 P
//   (make_inv_plan), hence the bound
//       rows * f * P / 2^32 < 3.5            rows <= 18 (N = 1024),  rows <= 16 (N = 2048)
//   (|acc| < 3.5 P 2^32 < 2^61 then holds with it: no int64 overflow).  The blind rotation's "|x| < 11.1 P, <= 6
//   products" (kernels.hip finish_inverse) is the same inequality for its own transforms.
// CRT bound (the chunk's true integer must be what the signed CRT returns).
//   A coefficient of S_i is a sum of rows * N products of a digit and a key word: |S_i| <= rows * N * (base - 1) * 2^31.
//   crt_signed_to_torus returns the centred integer exactly when it is below CRT_EXACT_LIMIT = 0.36 P0 P1 = 2^52.5
//   (ntt_field.hpp; the plain P0 P1 / 2 would do for canonical residues, the kernels' signed lazy residues need the
//   stricter limit), hence
//       rows * N * (base - 1) * 2^31 < CRT_EXACT_LIMIT.
//   With a chunk of ONE mask index (rows = t <= 32, base <= 16) the left side is at most 2^50.9: it always holds, while
//   all n t = 5,040 rows of P128 in one chunk (2^54.9) would wrap.  The chunk is therefore one mask index, and of the two
//   bounds it is the MAC bound that decides which decompositions are refused: t > 18 (N = 1024) or t > 16 (N = 2048).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntt_field.hpp"

namespace tfhe_hip {

constexpr int PACK_MAX_BASEBIT = 4;

// |outputs| / P of a forward transform of WaveNtt<logn> for inputs |x| <= x0 (the recurrence above; P the larger prime)
constexpr double pack_forward_bound(int logn, double x0) {
    const double P = (double)NTT_P[1], q = P / 4294967296.0;
    const int rb = logn - 6;
    const int stages[3] = {rb, rb, logn - 2 * rb};
    double b = x0 / P;
    for (int pass = 0; pass < 3; ++pass) {
        int cnt = stages[pass];
        for (; cnt >= 2; cnt -= 2) b = b + 1.0 + 3.0 * b * q;       // radix-4 step
        if (cnt) b = b + 0.5 + b * q;                               // radix-2 stage
    }
    return b;
}
constexpr int pack_logn(int N) { return N == 2048 ? 11 : 10; }
// MAC bound: `rows` products into one accumulator, then the reduction, must leave the inverse transform inputs below 4 P
constexpr bool pack_mac_ok(int N, int rows) {
    const double P = (double)NTT_P[1];
    return rows >= 1 && (double)rows * pack_forward_bound(pack_logn(N), (double)((1 << PACK_MAX_BASEBIT) - 1)) * P / 4294967296.0 < 3.5;
}
// CRT bound: the true integer of a chunk of `rows` rows stays inside the exact range of the signed CRT
constexpr bool pack_crt_ok(int N, int rows, int basebit) {
    // a 2^31 < L  <=>  a <= (L - 1) >> 31, which keeps the comparison inside 64 bits
    return rows >= 1 && (uint64_t)rows * (uint64_t)N * (uint64_t)((1 << basebit) - 1) <= ((CRT_EXACT_LIMIT - 1) >> 31);
}
// rows of one chunk of the kernel: one mask index
constexpr int pack_chunk_rows(int t) { return t; }
static_assert(pack_forward_bound(10, 15.0) < 6.1 && pack_forward_bound(11, 15.0) < 6.7, "forward bounds of ntt_wave.hpp");
static_assert(pack_mac_ok(1024, 18) && !pack_mac_ok(1024, 19) && pack_mac_ok(2048, 16) && !pack_mac_ok(2048, 17), "MAC bound");
static_assert(pack_crt_ok(2048, 32, 4) && !pack_crt_ok(1024, 5040, 2), "CRT bound: one mask index holds, a whole key does not");

// null if the kernel packs exactly under decomposition (t, basebit) of ring (N, k), else what is wrong with it
inline const char *pack_decomp_error(int N, int k, int t, int basebit) {
    if ((N != 1024 && N != 2048) || k != 1) return "the pack kernel is built for N = 1024 or 2048 and k = 1";
    if (basebit < 1 || basebit > PACK_MAX_BASEBIT || t < 1 || t * basebit > 32)
        return "packing digits must have 1..4 bits and t * basebit <= 32";
    if (!pack_mac_ok(N, pack_chunk_rows(t)))
        return "t rows of one mask index exceed what one 64-bit accumulator takes before its reduction (pack.hpp MAC bound)";
    if (!pack_crt_ok(N, pack_chunk_rows(t), basebit))
        return "t rows of one mask index exceed the exact range of the two-prime CRT (pack.hpp CRT bound)";
    return nullptr;
}
// prec of the definition: 2^(32 - (1 + basebit t)), and 0 where the digits cover all 32 bits (nothing to round)
constexpr uint32_t pack_prec_offset(int t, int basebit) { return t * basebit < 32 ? 1u << (31 - t * basebit) : 0u; }

// One pack.  samples: rows of `stride` words, the mask words of a sample first and its body at word n; sample j of the
// pack is row slots[j], or row j when slots is null.  img: the key's NTT image (launch_bk_transform of its raw rows
// [n][t][2][N] with nw = 2).  partial: ceil(n / idx_per_wg) * 2N words of scratch.  out: the 2N words of the result.
struct PackArgs {
    int32_t N, n, t, basebit, count;
    int32_t stride;
    int32_t idx_per_wg;             // mask indices per workgroup (>= 1)
    const int32_t *samples;
    const int32_t *slots;
    const uint32_t *img;
    const uint32_t *tw;             // the twiddle tables of a key of the same ring (DevKey::tw)
    int32_t *partial;
    int32_t *out;
};
inline int pack_groups(int n, int idx_per_wg) { return (n + idx_per_wg - 1) / idx_per_wg; }
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_pack(hipStream_t s, const PackArgs &a);

}  // namespace tfhe_hip
