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
// kernels.hip is not touched by this file.
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

}  // namespace

bool launch_ring_extract(hipStream_t s, const UnpackArgs &a) {
    // k = 1: a row is N mask words, the body and three words of padding
    if ((a.N != 1024 && a.N != 2048) || a.count < 1 || a.count > UNPACK_CHUNK || a.u_stride != a.N + 4 || !a.ring || !a.index ||
        !a.u_buf || (reinterpret_cast<uintptr_t>(a.u_buf) & 15u))
        return false;
    hipLaunchKernelGGL(ring_extract_kernel, dim3(a.count), dim3(256), 0, s, a);
    return true;
}

}  // namespace tfhe_hip
