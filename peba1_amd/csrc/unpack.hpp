// unpack.hpp -- the way in through ring samples (include/tfhe_hip.h "ring-encrypted inputs"): coefficient e of a TLWE
// sample under the ring key becomes the extracted sample Extract_e, which the key switch every gate ends with turns into
// an LWE sample under the LWE key.  Host-visible side of unpack.hip: what one extract launch works on, and the launcher.
//
// Extract_e of a sample (A, B), k = 1, wrapping mod 2^32 -- the header's definition, the one the multi-output bootstrap uses:
//     b = B[e],    a_i = A[e - i] for i <= e,    a_i = -A[N + e - i] for i > e
// The kernel writes row j of u_buf in the layout launch_keyswitch reads: the N mask words, the body at word N, zeros in
// the padding up to u_stride.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfhe_hip {

// the most samples one extract launch and the key switch behind it work on: bounds the extract scratch at
// UNPACK_CHUNK * u_stride words (33.7 MB at N = 1024) whatever the caller's count is
constexpr int UNPACK_CHUNK = 8192;

// One extract launch.  ring: nring samples of 2N words, the mask polynomial first, then the body.  index[j] = r N + e
// names coefficient e of sample r; the caller has checked 0 <= index[j] < nring N (the kernel does not).  u_buf: `count`
// rows of u_stride words, 16-byte aligned.
struct UnpackArgs {
    int32_t N, count, u_stride;
    const int32_t *ring;
    const int32_t *index;
    int32_t *u_buf;
};
// false, and nothing launched, for arguments outside what the kernel was built for
bool launch_ring_extract(hipStream_t s, const UnpackArgs &a);

}  // namespace tfhe_hip
