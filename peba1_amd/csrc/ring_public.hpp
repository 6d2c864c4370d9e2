// ring_public.hpp -- a ring sample times PUBLIC small-integer polynomials (include/tfhe_hip.h "ring sample times public
// polynomials"): q * (a, b) = (q a, q b) in Z[X]/(X^N + 1) mod 2^32, with no gadget, no decomposition and no TGSW sample.
// Host-visible side of ring_public.hip: the bounds the kernels rest on, as checked functions, and the two launchers.
// Shared by the gallery's constructor (public_host.cpp: a coefficient the CRT bound cannot take is refused there), the
// engine and the kernels.
//
// What the product kernel computes for one pair of a ring sample c and a public polynomial q, |q[j]| <= T:
//     out[u] = q(X) * c[u](X)        u = 0, 1, the words of c taken as signed 32-bit integers, mod 2^32
// through the two-prime NTT of ntt_wave.hpp: per prime and polynomial u one forward transform of c[u], ONE product with
// the canonical image word of q, its Montgomery reduction, one inverse transform; then the signed CRT.  Three bounds make
// that exact; all are derived here and none is tuned.
//
// Forward input bound.  The forward input is a full 32-bit word, not a digit.  pack_forward_bound's recurrence (pack.hpp)
// run from |x| <= 2^31 = 16.0 P ends at 31.1 P (N = 1024): past the 2^31 = 16.0 P an int32 representative holds.  So the
// word is REDUCED first, as bk_transform_kernel (kernels.hip) reduces key words: x <- mont_mul(x, R mod P) = x mod P with
// |x| < P (ntt_wave.hpp: |b w| / 2^32 + P/2 for any |b| < 2^31, 0 <= w < P), three multiplier-class instructions a word.
// From |x| < P the same recurrence gives public_forward_bound: below 7.6 P (N = 1024) / 8.2 P (N = 2048), the "inputs
// below P below 8.2 P" of ntt_wave.hpp, and far inside int32.
// Product bound.  One product of a transform output |x| < f P and a canonical image word 0 <= w < P: |x w| < f P^2 < 2^59,
// its Montgomery reduction is below f P^2 / 2^32 + P/2 < 0.76 P, and the inverse transform takes inputs below 4 P
// (make_inv_plan): the MAC bound of cmux.hpp with rows = 1 and this file's f.
// Gallery transform.  The forward input of the gallery's own transform is q itself, |q[j]| <= T <= 2^11: the digit bound of
// ntt_wave.hpp (cmux_forward_bound), then canonicalised like a key word.
// CRT bound (the true integer of an output coefficient must be what the signed CRT returns).  A coefficient of q c[u] is
// a sum of N products of a coefficient and a word:
//       |S| <= N * T * 2^31 < CRT_EXACT_LIMIT
// (ntt_field.hpp: 0.36 P0 P1 = 2^52.5).  T = public_max_coef(N) is the largest power of two that satisfies it: 2^11 at
// N = 1024 (2^52), 2^10 at N = 2048 (2^52).  All q[j] = -T against words 0x80000000 reach the left side exactly, at
// coefficient N - 1 (every term of that coefficient has the sign +).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntt_field.hpp"
#include "pack.hpp"
#include "ring_wave.hpp"

namespace tfhe_hip {

// the most ring samples or polynomials one raw launch takes
constexpr int32_t PUBLIC_MAX_COUNT = 1 << 16;
// the most polynomials a gallery holds (8 KB of image each: 8 GB)
constexpr int32_t PUBLIC_MAX_POLYS = 1 << 20;

// CRT bound: N T 2^31 < CRT_EXACT_LIMIT  <=>  N T <= (L - 1) >> 31, which keeps the comparison inside 64 bits
constexpr bool public_crt_ok(int N, int64_t T) {
    return (N == 1024 || N == 2048) && T >= 1 && T <= ((int64_t)1 << 31) && (uint64_t)N * (uint64_t)T <= ((CRT_EXACT_LIMIT - 1) >> 31);
}
// the largest power of two the CRT bound takes (0 for a ring the kernels are not built for)
constexpr int32_t public_max_coef(int N) {
    int64_t T = 0;
    for (int64_t t = 1; t <= ((int64_t)1 << 30) && public_crt_ok(N, t); t *= 2) T = t;
    return (int32_t)T;
}
static_assert(public_max_coef(1024) == 2048 && public_max_coef(2048) == 1024, "T = 2^11 at N = 1024, 2^10 at N = 2048");
static_assert(public_crt_ok(1024, 2048) && !public_crt_ok(1024, 4096) && public_crt_ok(2048, 1024) && !public_crt_ok(2048, 2048),
              "CRT bound: T holds, 2 T does not");

// |outputs| / P of a forward transform of WaveNtt<logn> on words reduced to |x| < P
constexpr double public_forward_bound(int logn) { return pack_forward_bound(logn, (double)NTT_P[1]); }
// the same from the unreduced word, |x| <= 2^31: why the word is reduced first
constexpr double public_forward_bound_unreduced(int logn) { return pack_forward_bound(logn, 2147483648.0); }
// product bound: one product, then the reduction, must leave the inverse transform inputs below 4 P
constexpr bool public_product_ok(int N) {
    const double P = (double)NTT_P[1];
    return public_forward_bound(pack_logn(N)) * P / 4294967296.0 + 0.5 < 4.0;
}
static_assert(public_forward_bound(10) < 7.6 && public_forward_bound(11) < 8.2, "forward bounds for inputs below P (ntt_wave.hpp: below 8.2 P)");
static_assert(public_forward_bound(11) * (double)NTT_P[1] < 2147483648.0, "a transform of reduced words stays inside int32");
static_assert(public_forward_bound_unreduced(10) * (double)NTT_P[1] > 2147483648.0, "a transform of unreduced words would not");
static_assert(public_product_ok(1024) && public_product_ok(2048), "product bound");
// the gallery transform's input: |q| <= T <= 2^11, the digit bound pack_forward_bound confirms (cmux.hpp cmux_forward_bound)
static_assert(public_max_coef(1024) <= 2048 && pack_forward_bound(10, 2048.0) < 6.1 && pack_forward_bound(11, 2048.0) < 6.7,
              "forward bounds of ntt_wave.hpp for |x| <= 2^11");

// The gallery image: R public polynomials polys[R][N] (device words, |coefficient| <= public_max_coef(N): the caller has
// checked it) -> img[R][prime 2][N] canonical residues in the order the product kernel loads them (word 256 g + 4 lane + e
// = register 4 g + e of `lane` in layout L2, as kernels.hip bk_transform_kernel stores a key polynomial), scaled by
// scale[prime] (engine.cpp make_twiddles).  8 KB a polynomial.
struct PublicImageArgs {
    int32_t N, count;
    const int32_t *polys;
    uint32_t *img;
    const uint32_t *tw;             // the twiddle tables of the ring (engine.cpp make_twiddles)
    uint32_t scale[2];
};
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_public_image(hipStream_t s, const PublicImageArgs &a);

// One launch of `count` workgroups: workgroup g multiplies the ring sample at ring[g * ring_stride] (2N words; stride 0:
// every workgroup reads the same sample) by the polynomial whose image is img[(g * img_step) * 2N] (img_step 0: every
// workgroup the same polynomial, 1: consecutive ones).
// rows.u_buf != null: the rows Extract_(e width)(q_g * c_g) of ring_wave.hpp RingRows, passing ring_rows_error.  out !=
// null: the full products out[g * 2N] as well (alone when u_buf is null).  out overlaps no input.
struct PublicArgs {
    int32_t N, count;
    int32_t img_step;               // 0 or 1
    int64_t ring_stride;            // 0, or at least 2N and a multiple of 4
    const int32_t *ring;
    const uint32_t *img;            // the image of workgroup 0's polynomial
    const uint32_t *tw;
    int32_t *out;
    RingRows rows;
};
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_public(hipStream_t s, const PublicArgs &a);

// ---- sums of products over several ring samples (include/tfhe_hip.h "public products over several ring samples") ----
// out[u] = sum_(t < K) q_t(X) * c_t[u](X): K ring samples c_t against the K polynomials of one GROUP of the gallery, the
// sum taken in the NTT domain -- per prime and output polynomial u, K forward transforms, K products with an image word
// into one 64-bit accumulator, ONE Montgomery reduction, ONE inverse transform -- then the signed CRT once.  A public
// matrix-vector product where public_kernel is a diagonal one.  The forward input bound and the gallery transform are
// those above, per term; the other two bounds change.
// MAC bound (how many products one int64 accumulator takes before its reduction), cmux.hpp's with this file's f.
//   K products of a transform output |x| < f P (f = public_forward_bound: 7.6 / 8.2) and a canonical image word
//   0 <= w < P: |acc| < K f P^2; its Montgomery reduction is below K f P^2 / 2^32 + P/2, and the inverse transform takes
//   inputs below 4 P (make_inv_plan), hence
//       K * f * P / 2^32 < 3.5               K <= 14 (N = 1024),  K <= 13 (N = 2048)
//   (|acc| < 3.5 P 2^32 < 2^61 then holds with it: no int64 overflow).  PUBLIC_MAX_TERMS is the largest power of two both
//   rings take: 8.  K = 1 is public_product_ok, and the kernel then computes public_kernel's words (one product, the same
//   reduction).
// CRT bound.  A coefficient of sum_t q_t c_t[u] is a sum of K N products of a coefficient and a word:
//       |S| <= N * (sum_t max|q_t|) * 2^31 < CRT_EXACT_LIMIT
//   so the per-term maxima of a group may sum to T = public_max_coef(N), the power of two a single polynomial is held to:
//   a group is held to what ONE polynomial is, and K = 1 changes nothing.  The gallery keeps max|q| of every polynomial
//   from its construction and the host caller adds them up per group before the device is touched (public_host.cpp).
//   All q_t[j] = -T / K against words 0x80000000 reach N T 2^31 exactly, at coefficient N - 1.
constexpr int PUBLIC_MAX_TERMS = 8;
constexpr bool public_sum_mac_ok(int N, int terms) {
    const double P = (double)NTT_P[1];
    return terms >= 1 && (double)terms * public_forward_bound(pack_logn(N)) * P / 4294967296.0 < 3.5;
}
// the most terms the MAC bound takes
constexpr int public_sum_mac_terms(int N) {
    int K = 0;
    while (K < 64 && public_sum_mac_ok(N, K + 1)) ++K;
    return K;
}
constexpr bool public_sum_crt_ok(int N, int terms, int64_t coef_sum) {
    return terms >= 1 && terms <= PUBLIC_MAX_TERMS && coef_sum >= 0 && coef_sum <= public_max_coef(N) &&
           (coef_sum == 0 || public_crt_ok(N, coef_sum));
}
static_assert(public_sum_mac_terms(1024) == 14 && public_sum_mac_terms(2048) == 13, "MAC bound: the exact figures");
static_assert(public_sum_mac_ok(1024, PUBLIC_MAX_TERMS) && public_sum_mac_ok(2048, PUBLIC_MAX_TERMS) &&
                  (!public_sum_mac_ok(1024, 2 * PUBLIC_MAX_TERMS) || !public_sum_mac_ok(2048, 2 * PUBLIC_MAX_TERMS)) &&
                  (PUBLIC_MAX_TERMS & (PUBLIC_MAX_TERMS - 1)) == 0,
              "PUBLIC_MAX_TERMS is the largest power of two the MAC bound takes at both ring sizes");
static_assert((double)PUBLIC_MAX_TERMS * public_forward_bound(11) * (double)NTT_P[1] * (double)NTT_P[1] < 2305843009213693952.0,
              "the accumulator stays below 2^61");
static_assert(public_sum_crt_ok(1024, 8, 2048) && !public_sum_crt_ok(1024, 8, 2049) && public_sum_crt_ok(2048, 8, 1024) &&
                  !public_sum_crt_ok(2048, 8, 1025) && !public_sum_crt_ok(1024, 9, 1) && !public_sum_crt_ok(1024, 0, 1),
              "CRT bound of a group: the sum of the maxima is held to one polynomial's T");

// One launch of `count` workgroups: workgroup g forms sum_(t < terms) q_(g terms + t) * c_t from the `terms` ring samples at
// ring[t * 2N] (every workgroup reads the same ones) and the polynomials whose images start at img[(g terms) * 2N].
// rows / out: as PublicArgs, entry e of workgroup g being row g S + e.  out overlaps no input.
struct PublicSumArgs {
    int32_t N, count, terms;        // terms in 1 .. PUBLIC_MAX_TERMS
    const int32_t *ring;            // [terms][2N]
    const uint32_t *img;            // the image of workgroup 0's first polynomial
    const uint32_t *tw;
    int32_t *out;
    RingRows rows;
};
// false, and nothing launched, for arguments outside what the kernel was built and bounded for
bool launch_public_sum(hipStream_t s, const PublicSumArgs &a);

}  // namespace tfhe_hip
