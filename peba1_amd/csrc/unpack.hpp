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

// A seed-compressed ring sample (include/tfhe_hip.h "seed-compressed packing keys and ring samples") is a record of
// RING_SEED_WORDS + N words: the mask seed (ChaCha20 key[8], nonce[2]), then the body.  Mask word j of the sample is word j
// of the stream of its own seed (expand.hpp: word 2 (j mod 8) + 1 of block j / 8).
constexpr int RING_SEED_WORDS = 10;
// One seeded extract launch: as UnpackArgs, with ring = nring records of RING_SEED_WORDS + N words.  The rows it writes
// are those launch_ring_extract writes from the expanded samples.
struct UnpackSeededArgs {
    int32_t N, count, u_stride;
    const int32_t *ring;
    const int32_t *index;
    int32_t *u_buf;
};
bool launch_ring_extract_seeded(hipStream_t s, const UnpackSeededArgs &a);

}  // namespace tfhe_hip
