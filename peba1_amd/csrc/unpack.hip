// unpack.hip -- the sample extract of ring-encrypted inputs on gfx950 (unpack.hpp has the definition).
//
//   ring_extract_kernel   one workgroup of four wave64 per output row.  A lane owns 16-byte groups of four consecutive
//                         words of the row: it reads the mask polynomial descending from A[e - 4g] -- past the wrap from
//                         the top of the polynomial, negated -- and writes the group with one 16-byte store.  The last
//                         group of a row is the body B[e] and three zeros of padding (u_stride = N + 4 for k = 1).
//
// Write-bound: a row is 4 KB out for four words in per lane, and the 8 KB of a ring sample are read by up to N rows, so
// they come from the L2 after the first; no LDS staging (the descending reads of a wave cover one contiguous KB).  Nothing
// is read-modified: every word of a row, padding included, is written exactly once, with vector stores.
//
//   ring_extract_seeded_kernel   the same rows from seed-compressed samples (RING_SEED_WORDS + N words: seed, body).  The
//                         mask polynomial never exists in global memory: the workgroup reads the ten seed words of its
//                         sample (uniform: scalar loads), lane b < N/8 computes ChaCha20 block b with the block function
//                         expand.hip uses (chacha_device.hpp) and puts its eight mask words into LDS with two 16-byte
//                         writes -- N words, 4 KB at N = 1,024 and 8 KB at 2,048 -- and after ONE barrier (LDS counter
//                         drained, then s_barrier) the row leaves exactly as above, A[] being the LDS copy.
//                         One row per workgroup per generated mask.  The rows of a launch name samples in any order, so
//                         serving R rows from one mask needs runs of equal samples to be found first and leaves count / R
//                         workgroups to write the same bytes; what it would save is small: N/8 blocks of about 1,050 VALU
//                         operations are 1.3e5 lane-operations a row at N = 1,024, 1.4e8 for 1,024 rows -- microseconds on
//                         65,536 lanes -- beside 4 KB of stores a row, and the grid, the store pattern and the bounds stay
//                         those of ring_extract_kernel.  Half of a workgroup's lanes hold a block at N = 1,024, all at 2,048.
//                         The descending 4-word reads of neighbouring lanes lie 16 bytes apart: 4-way bank conflicts, 16
//                         LDS passes per wave and row, nothing beside the ChaCha rounds in front of them.
//
// kernels.hip is not touched by this file.
#include "chacha_device.hpp"
#include "unpack.hpp"

namespace tfhe_hip {

namespace {

__global__ __launch_bounds__(256) void ring_extract_kernel(UnpackArgs a) {
    const int N = a.N, j = blockIdx.x;                    // the grid is `count` workgroups
    const int idx = a.index[j];
    const int r = idx >> (31 - __builtin_clz(N)), e = idx & (N - 1);       // N is a power of two (the launcher checks)
    const uint32_t *A = reinterpret_cast<const uint32_t *>(a.ring) + (size_t)r * 2 * N;
    const uint32_t *B = A + N;
    uint4 *row = reinterpret_cast<uint4 *>(a.u_buf + (size_t)j * a.u_stride);
    const int groups = N / 4;                             // mask groups; group `groups` is (b, 0, 0, 0)
    for (int g = threadIdx.x; g <= groups; g += 256) {
        uint4 w;
        if (g < groups) {
            uint32_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int d = e - (4 * g + c);
                v[c] = d >= 0 ? A[d] : 0u - A[d + N];
            }
            w = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
            w = make_uint4(B[e], 0u, 0u, 0u);
        }
        row[g] = w;
    }
}

// data exchanged through LDS only: the LDS counter is drained, nothing else (ntt_wave.hpp lds_barrier)
__device__ __forceinline__ void unpack_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(256) void ring_extract_seeded_kernel(UnpackSeededArgs a) {
    extern __shared__ uint32_t A[];                       // the sample's N mask words (the launcher passes N * 4 bytes)
    const int N = a.N, j = blockIdx.x;                    // the grid is `count` workgroups
    const int idx = a.index[j];
    const int r = idx >> (31 - __builtin_clz(N)), e = idx & (N - 1);
    const uint32_t *rec = reinterpret_cast<const uint32_t *>(a.ring) + (size_t)r * (RING_SEED_WORDS + N);
    const uint32_t *B = rec + RING_SEED_WORDS;
    ExpandSeed seed;
#pragma unroll
    for (int i = 0; i < 8; ++i) seed.key[i] = rec[i];
    seed.nonce[0] = rec[8];
    seed.nonce[1] = rec[9];
    for (int b = threadIdx.x; b < N / 8; b += 256) {
        uint32_t w[8];
        chacha_mask_words(seed, (uint64_t)b, w);
        uint4 *dst = reinterpret_cast<uint4 *>(A + 8 * b);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    unpack_lds_barrier();
    uint4 *row = reinterpret_cast<uint4 *>(a.u_buf + (size_t)j * a.u_stride);
    const int groups = N / 4;                             // mask groups; group `groups` is (b, 0, 0, 0)
    for (int g = threadIdx.x; g <= groups; g += 256) {
        uint4 w;
        if (g < groups) {
            uint32_t v[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int d = e - (4 * g + c);
                v[c] = d >= 0 ? A[d] : 0u - A[d + N];
            }
            w = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
            w = make_uint4(B[e], 0u, 0u, 0u);
        }
        row[g] = w;
    }
}

}  // namespace

bool launch_ring_extract_seeded(hipStream_t s, const UnpackSeededArgs &a) {
    // k = 1, as launch_ring_extract; N / 8 blocks fill the N words of LDS (8 KB at most)
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > UNPACK_CHUNK || a.u_stride != a.N + 4 || !a.ring || !a.index ||
        !a.u_buf || (reinterpret_cast<uintptr_t>(a.u_buf) & 15u))
        return false;
    hipLaunchKernelGGL(ring_extract_seeded_kernel, dim3(a.count), dim3(256), (size_t)a.N * 4, s, a);
    return true;
}

bool launch_ring_extract(hipStream_t s, const UnpackArgs &a) {
    // k = 1: a row is N mask words, the body and three words of padding
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > UNPACK_CHUNK || a.u_stride != a.N + 4 || !a.ring || !a.index ||
        !a.u_buf || (reinterpret_cast<uintptr_t>(a.u_buf) & 15u))
        return false;
    hipLaunchKernelGGL(ring_extract_kernel, dim3(a.count), dim3(256), 0, s, a);
    return true;
}

}  // namespace tfhe_hip
