// expand.hip -- the public masks of a seed-compressed cloud key, regenerated on gfx950 (expand.hpp has the definition).
//
//   chacha_mask_words   (chacha_device.hpp, shared with unpack.hip) one lane computes one ChaCha20 block in registers: 16
//                       words of state, 20 rounds of add / xor / rotate, the feed-forward; the eight odd words are the
//                       block's mask words (Rng::torus() takes the high half of each 64-bit draw).
//   expand_bk_kernel    a lane per group of eight consecutive words of the raw [rows][k+1][N] staging buffer: a mask
//                       group is one block, a body group eight uploaded words; either leaves as two 16-byte stores.  A
//                       polynomial is N/8 >= 128 groups, so a wave never holds both kinds.
//   expand_ksk_kernel   a lane per block of the KSK's part of the stream; its eight words go to (row, q) = (m / n, m % n)
//                       of the compact layout -- n is generally no multiple of 8 (630), so a block falls into two rows, or
//                       nine when n = 1.  Behind the blocks, a lane per row writes the body at word n and the padding.
//
// Compute-bound on integer VALU (about 350 add / xor / rotate triples a block) with 32 bytes out per lane.  Every word of both
// images is written here exactly once, with plain vector stores; the KSK's zero row is cleared by the caller.
//
//   lwe_expand_kernel   seed-compressed LWE sample arrays (expand.hpp LweExpandArgs): one workgroup of four wave64 per result
//                       row, which is sample s = index[j] of the record.  The row's stream words [s n, s n + n) lie in blocks
//                       floor(s n / 8) .. floor((s n + n - 1) / 8): at most ceil(n / 8) + 1 = 129 of them at n = 1,024.  Lane b
//                       below that count computes block b and puts the words that fall inside the row into LDS; lanes 192 ..
//                       195 put the body at word n and the zeros up to the slot stride behind it.  After ONE barrier the row
//                       -- stride words, 4,112 bytes at most -- leaves LDS for its pool slot in 16-byte groups, one store a
//                       lane (two for lane 0 when stride / 4 = 257).  The staging is what the layout asks for: s n mod 8 is
//                       arbitrary (630 mod 8 = 6), so a block's eight words never line up with the slot's 16-byte groups,
//                       and a lane that stored its own words would store single words at odd offsets.  No expanded array
//                       exists in global memory: the slot is the only destination.
//                       Counted per row at n = 630: 79 or 80 blocks of about 1,050 VALU operations = 8.4e4 lane-operations
//                       in two of the four waves, against 2,528 bytes stored (158 16-byte groups); 1,024 rows are 8.6e7
//                       lane-operations and 2.6 MB of stores.  A sample named twice is computed twice: finding repeats
//                       costs more than the blocks they would save.
//                       Bounds: s < 2^20 and n <= 1,024, so s n + n <= 2^30 and 32-bit index arithmetic is exact (the
//                       launcher refuses other n; the caller has checked every index and slot); LDS words touched are
//                       i < n by the test in front of each write, and n .. stride - 1 <= n + 3 by lanes 192 .. 195; the
//                       global stores cover words 0 .. stride - 1 of the row's own slot and nothing else.
//
// kernels.hip is not touched by this file.
#include "chacha_device.hpp"
#include "expand.hpp"

namespace tfhe_hip {

namespace {

__global__ __launch_bounds__(256) void expand_bk_kernel(ExpandBkArgs a) {
    const uint32_t gpp = (uint32_t)a.N / 8;                   // groups per polynomial
    const uint64_t groups = (uint64_t)a.rows * (uint32_t)(a.k + 1) * gpp;
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= groups) return;
    const uint64_t poly = g / gpp;
    const uint32_t jg = (uint32_t)(g % gpp);
    const uint64_t row = poly / (uint32_t)(a.k + 1);
    const uint32_t u = (uint32_t)(poly % (uint32_t)(a.k + 1));
    uint4 lo, hi;
    if (u < (uint32_t)a.k) {
        uint32_t w[8];
        chacha_mask_words(a.seed, (row * (uint32_t)a.k + u) * gpp + jg, w);
        lo = make_uint4(w[0], w[1], w[2], w[3]);
        hi = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.body + row * (uint32_t)a.N + (size_t)jg * 8);
        lo = src[0];
        hi = src[1];
    }
    uint4 *dst = reinterpret_cast<uint4 *>(a.raw + g * 8);
    dst[0] = lo;
    dst[1] = hi;
}

__global__ __launch_bounds__(256) void expand_ksk_kernel(ExpandKskArgs a) {
    const uint64_t words = (uint64_t)a.rows * (uint32_t)a.n;          // mask words of the KSK
    const uint64_t blocks = (words + 7) / 8;
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t *ksk = reinterpret_cast<uint32_t *>(a.ksk);
    if (idx < blocks) {
        uint32_t w[8];
        chacha_mask_words(a.seed, a.first_block + idx, w);
        uint64_t m = idx * 8, row = m / (uint32_t)a.n;
        uint32_t q = (uint32_t)(m % (uint32_t)a.n);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (m + c < words) ksk[row * (uint32_t)a.stride + q] = w[c];
            if (++q == (uint32_t)a.n) { q = 0; ++row; }
        }
    } else if (idx - blocks < (uint64_t)a.rows) {
        const uint64_t row = idx - blocks;
        uint32_t *tail = ksk + row * (uint32_t)a.stride;
        tail[a.n] = (uint32_t)a.body[row];
        for (int q = a.n + 1; q < a.stride; ++q) tail[q] = 0u;
    }
}

__global__ __launch_bounds__(256) void lwe_expand_kernel(LweExpandArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lwe_row[];   // the row as its slot will hold it: stride words
    const uint32_t n = (uint32_t)a.n, stride = (uint32_t)a.stride, j = blockIdx.x;     // the grid is `count` workgroups
    const uint32_t s = (uint32_t)a.index[j];
    const uint32_t first = s * n;                                        // the row's first stream word, below 2^30
    const uint32_t b0 = first / 8, nblocks = (first + n - 1) / 8 - b0 + 1;             // at most ceil(n / 8) + 1 <= 129
    if (threadIdx.x < nblocks) {
        ExpandSeed seed;
#pragma unroll
        for (int i = 0; i < 8; ++i) seed.key[i] = a.seed[i];
        seed.nonce[0] = a.seed[8];
        seed.nonce[1] = a.seed[9];
        uint32_t w[8];
        chacha_mask_words(seed, (uint64_t)(b0 + threadIdx.x), w);
        const uint32_t i0 = (b0 + threadIdx.x) * 8 - first;              // wraps below zero in front of the row: fails i < n
#pragma unroll
        for (uint32_t c = 0; c < 8; ++c)
            if (i0 + c < n) lwe_row[i0 + c] = w[c];
    } else if (threadIdx.x >= 192) {
        const uint32_t q = n + (threadIdx.x - 192);                      // the body, then the padding an import leaves zero
        if (q < stride) lwe_row[q] = q == n ? (uint32_t)a.body[a.gathered ? j : s] : 0u;
    }
    __syncthreads();
    const size_t at = a.slots ? (size_t)a.slots[j] : (size_t)j;
    uint4 *dst = reinterpret_cast<uint4 *>(a.rows + at * stride);
    const uint4 *src = reinterpret_cast<const uint4 *>(lwe_row);
    for (uint32_t g = threadIdx.x; g < stride / 4; g += 256) dst[g] = src[g];
}

__global__ __launch_bounds__(256) void expand_masks_kernel(ExpandSeed seed, uint64_t first_word, uint32_t count, uint32_t *out) {
    const uint64_t counter = first_word / 8 + ((uint64_t)blockIdx.x * 256 + threadIdx.x);     // base + block index, 64-bit
    if (counter > (first_word + count - 1) / 8) return;
    uint32_t w[8];
    chacha_mask_words(seed, counter, w);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint64_t m = counter * 8 + c;
        if (m >= first_word && m - first_word < count) out[m - first_word] = w[c];
    }
}

bool aligned16(const void *p) { return p && !(reinterpret_cast<uintptr_t>(p) & 15u); }

}  // namespace

bool launch_lwe_expand(hipStream_t s, const LweExpandArgs &a) {
    // a row is n mask words, the body and the padding up to the slot stride; ceil(n / 8) + 1 blocks stay below lane 192
    if (a.n < 1 || a.n > LWE_EXPAND_MAX_N || a.stride != ((a.n + 4) & ~3) || a.count < 1 || a.count > LWE_EXPAND_CHUNK || !a.seed ||
        !a.body || !a.index || !aligned16(a.rows))
        return false;
    hipLaunchKernelGGL(lwe_expand_kernel, dim3(a.count), dim3(256), (size_t)a.stride * 4, s, a);
    return true;
}

bool launch_expand_bk(hipStream_t s, const ExpandBkArgs &a) {
    if (a.rows < 1 || a.k < 1 || a.N < 8 || (a.N & 7) || !aligned16(a.body) || !aligned16(a.raw)) return false;
    const uint64_t groups = (uint64_t)a.rows * (uint32_t)(a.k + 1) * ((uint32_t)a.N / 8);
    if ((groups + 255) / 256 > 0x7fffffffull) return false;
    hipLaunchKernelGGL(expand_bk_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, s, a);
    return true;
}

bool launch_expand_ksk(hipStream_t s, const ExpandKskArgs &a) {
    if (a.rows < 1 || a.n < 1 || a.stride < a.n + 1 || (a.first_block >> 60) || !a.body || !a.ksk) return false;
    const uint64_t lanes = ((uint64_t)a.rows * (uint32_t)a.n + 7) / 8 + (uint64_t)a.rows;
    if ((lanes + 255) / 256 > 0x7fffffffull) return false;
    hipLaunchKernelGGL(expand_ksk_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, a);
    return true;
}

bool launch_expand_masks(hipStream_t s, const ExpandSeed &seed, int64_t first_word, int32_t count, uint32_t *out) {
    if (first_word < 0 || (first_word >> 60) || count < 1 || count > EXPAND_MASKS_MAX || !out) return false;
    const uint64_t blocks = ((uint64_t)first_word + (uint32_t)count - 1) / 8 - (uint64_t)first_word / 8 + 1;
    hipLaunchKernelGGL(expand_masks_kernel, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, seed, (uint64_t)first_word,
                       (uint32_t)count, out);
    return true;
}

}  // namespace tfhe_hip
