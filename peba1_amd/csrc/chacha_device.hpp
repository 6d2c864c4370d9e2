// chacha_device.hpp -- the block function of the mask stream on the device (expand.hpp has the stream's definition): one
// lane computes one ChaCha20 block in registers and keeps its eight mask words.  Device code only; included by expand.hip
// (the cloud and packing keys' masks) and unpack.hip (the masks of seed-compressed ring samples), so that every public mask
// on the card comes from one function.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "expand.hpp"

namespace tfhe_hip {

#define EXPAND_QR(a, b, c, d)                                   \
    a += b; d = __builtin_rotateleft32(d ^ a, 16);              \
    c += d; b = __builtin_rotateleft32(b ^ c, 12);              \
    a += b; d = __builtin_rotateleft32(d ^ a, 8);               \
    c += d; b = __builtin_rotateleft32(b ^ c, 7)

// the eight mask words of block `counter`: words 1, 3, ..., 15 of the ChaCha20 block (RFC 8439 2.3 with the original
// 64-bit counter / 64-bit nonce split: the counter's high half is word 13)
__device__ __forceinline__ void chacha_mask_words(const ExpandSeed &s, uint64_t counter, uint32_t w[8]) {
    const uint32_t c0 = (uint32_t)counter, c1 = (uint32_t)(counter >> 32);
    uint32_t x0 = 0x61707865u, x1 = 0x3320646eu, x2 = 0x79622d32u, x3 = 0x6b206574u;
    uint32_t x4 = s.key[0], x5 = s.key[1], x6 = s.key[2], x7 = s.key[3];
    uint32_t x8 = s.key[4], x9 = s.key[5], x10 = s.key[6], x11 = s.key[7];
    uint32_t x12 = c0, x13 = c1, x14 = s.nonce[0], x15 = s.nonce[1];
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        EXPAND_QR(x0, x4, x8, x12); EXPAND_QR(x1, x5, x9, x13); EXPAND_QR(x2, x6, x10, x14); EXPAND_QR(x3, x7, x11, x15);
        EXPAND_QR(x0, x5, x10, x15); EXPAND_QR(x1, x6, x11, x12); EXPAND_QR(x2, x7, x8, x13); EXPAND_QR(x3, x4, x9, x14);
    }
    w[0] = x1 + 0x3320646eu; w[1] = x3 + 0x6b206574u;
    w[2] = x5 + s.key[1];    w[3] = x7 + s.key[3];
    w[4] = x9 + s.key[5];    w[5] = x11 + s.key[7];
    w[6] = x13 + c1;         w[7] = x15 + s.nonce[1];
}
#undef EXPAND_QR

}  // namespace tfhe_hip
