// ring_rotate.hpp -- the blind rotation of an ENCRYPTED ring sample by an LWE sample under the cloud key
// (include/tfhe_hip.h "ring LUT bootstrap"): host-visible side of ring_rotate.hip, the argument of its launch and the
// checks the launcher makes.
//
// What the kernel computes for rotation j, with c = ring[ring_index[j]] and (alpha_0 .. alpha_(n-1), beta) its LWE sample:
//     abar_i = round(alpha_i 2N / 2^32) mod 2N,  bbar likewise from beta        (the gate path's modulus switch)
//     ACC_0     = X^(-bbar) c                                                     both polynomials
//     ACC_(i+1) = CMUX(BK_i, X^(abar_i) ACC_i, ACC_i)                             i < n; a step with abar_i = 0 is SKIPPED
// with (X^(-r) c)[u][j] = c[u][(j + r) mod 2N] for an index below N and -c[u][index - N] from N on, 0 <= r < 2N -- cmux.hpp's
// rotation convention continued past N, where it negates -- and X^(abar) = X^(-(2N - abar)).  The CMUX is cmux.hpp's: the
// offset decomposition of the rotated difference, (k+1) l forward transforms, the 64-bit multiply-accumulate against row
// block i of the cloud key's NTT image (kernels.hpp DevKey::bk_img, [n][(k+1) l][prime][2][N]: a selector's image with n
// bits), one reduction, the inverse transforms, the signed CRT, the sum added to ACC_i.  A skipped step and a computed one
// leave the same words: the difference is zero, the digits of the offset alone are ((Bg/2) - Bg/2) = 0, the sum is zero.
//
// Bounds.  There is no new magnitude analysis.  One step is ONE CMUX of cmux.hpp on the operand pair (X^(abar) ACC_i,
// ACC_i), and cmux.hpp's two bounds take the operands as arbitrary 32-bit words: the digits of ANY word are in
// [-Bg/2, Bg/2) (forward input bound, MAC bound), the row words are any 32-bit words (CRT bound).  The accumulator goes
// back to plain torus words mod 2^32 after every step -- nothing is carried between steps in the NTT domain --, so the
// n steps are n independent instances of those bounds, whatever ACC_i has become.  cmux_gadget_error is therefore the whole
// admission test, and every gadget a cloud key is accepted with passes it (tests/test_select_cpu.py enumerates them).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cmux.hpp"

namespace tfhe_hip {

// the LWE dimensions a cloud key is accepted with (engine.cpp unsupported_reason): the kernel's abar vector is sized for it
constexpr int ROTATE_MAX_LWE_N = 1024;
// the most rotations of one launch (a grid of that many workgroups)
constexpr int ROTATE_MAX_COUNT = 1 << 16;

// what the argument above rests on: the accumulators take the rows of every admitted gadget, and abar < 2N fits 16 bits
static_assert(cmux_mac_ok(1024, 18) && cmux_mac_ok(2048, 16), "rows one accumulator takes (cmux.hpp MAC bound)");
static_assert(2 * 2048 <= 65536, "abar and bbar are kept as 16-bit words");

// One launch: `count` rotations, workgroup j on ring sample ring[ring_index[j] * 2N] (ring_index null: sample j) by the LWE
// sample at lwe[lwe_index[j] * lwe_stride] (lwe_index null: sample j; n mask words, then the body) -- a pool and a slot
// list, or a caller's array.  out != null: ACC_n of rotation j at out[j * 2N] (16-byte aligned); else rows.u_buf: the row
// Extract_0(ACC_n) as row j of u_buf in ring_extract_kernel's layout (RingRows with width = N, M = count).  The caller has
// checked ring_index against the samples `ring` holds.  img, tw: the cloud key's image and twiddle tables, as they rest.
struct RingRotateArgs {
    int32_t N, l, Bgbit, n, count;
    uint32_t offset;                // sum_p (Bg/2) 2^(32 - p Bgbit): the decomposition's offset
    int64_t lwe_stride;
    const int32_t *ring, *ring_index;
    const int32_t *lwe, *lwe_index;
    const uint32_t *img, *tw;
    int32_t *out;
    RingRows rows;
};

// null if the launcher takes these arguments, else what is wrong with them
inline const char *ring_rotate_error(const RingRotateArgs &a) {
    if (const char *why = cmux_gadget_error(a.N, 1, a.l, a.Bgbit)) return why;
    if (a.n < 1 || a.n > ROTATE_MAX_LWE_N) return "the LWE dimension must be in 1..1024";
    if (a.count < 1 || a.count > ROTATE_MAX_COUNT) return "a launch takes 1..65536 rotations";
    if (a.lwe_stride < (int64_t)a.n + 1) return "an LWE sample is n + 1 words";
    if (!a.ring || !a.lwe || !a.img || !a.tw) return "null operand";
    if ((a.out != nullptr) == (a.rows.u_buf != nullptr)) return "one destination: ring samples or rows";
    if ((reinterpret_cast<uintptr_t>(a.ring) | reinterpret_cast<uintptr_t>(a.out) | reinterpret_cast<uintptr_t>(a.rows.u_buf)) & 15u)
        return "ring words and destinations are 16-byte aligned";
    if (a.rows.u_buf) {
        if (a.rows.width != a.N || a.rows.M != a.count) return "a rotation leaves one row: width = N, M = count";
        return ring_rows_error(a.N, a.count, a.rows.M, a.rows.width, a.rows.u_stride);
    }
    return nullptr;
}

// false, and nothing launched, for arguments ring_rotate_error refuses
bool launch_ring_rotate(hipStream_t s, const RingRotateArgs &a);

}  // namespace tfhe_hip
