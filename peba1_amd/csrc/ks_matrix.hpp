// ks_matrix.hpp -- the key switch of wide levels as an int8 matrix product (ks_matrix.hip), host-visible part.
#pragma once
#include "kernels.hpp"

namespace tfhe_hip {

// A KSK word as four signed bytes with sum_p s[p] 2^(8p) = w (mod 2^32): a byte of 128 or more carries into the next,
// the carry out of byte 3 is dropped.
__host__ __device__ inline void ks_byte_planes(uint32_t w, int8_t s[4]) {
    uint32_t carry = 0;
    for (int p = 0; p < 4; ++p) {
        const uint32_t t = ((w >> (8 * p)) & 0xffu) + carry;     // 0 .. 256
        carry = t >= 128u ? 1u : 0u;
        s[p] = (int8_t)(int)(t - (carry << 8));
    }
}

// Gates of a workgroup's tile, output words of a column tile, and the waves of a workgroup (each takes 1 / KSM_WAVES of the
// input coefficients, in blocks of KSM_CHUNK).
constexpr int KSM_GATES = 64, KSM_WORDS = 32, KSM_WAVES = 8, KSM_CHUNK = 32;

// the shapes the matrix form is built for: digits of base 4 in 8 positions, coefficient ranges of whole chunks per wave
inline bool ks_matrix_shape_ok(int nin, int ks_t, int ks_basebit) {
    return ks_t == 8 && ks_basebit == 2 && nin > 0 && nin % (KSM_WAVES * KSM_CHUNK) == 0;
}
// The byte-plane image of a key: [column tile][coefficient i][plane p][lane 64][16 bytes], 4 KB per (tile, i).
inline size_t ks_matrix_image_bytes(int nin, int ct_stride) {
    return (size_t)((ct_stride + KSM_WORDS - 1) / KSM_WORDS) * (size_t)nin * 4 * 64 * 16;
}

// image <- the resident KSK (key.ksk, rows of p.ct_stride words).  False and no launch for a shape the form is not built for.
bool launch_ksk_planes(hipStream_t s, const DevParams &p, const DevKey &key, uint8_t *image);
// The key switches of `count` gates straight into their pool slots: no partial sums, no reduce launch.
bool launch_keyswitch_matrix(hipStream_t s, const DevParams &p, const uint8_t *image, const int32_t *u_buf,
                             const KsDesc *descs, int count, int32_t *pool);

}  // namespace tfhe_hip
