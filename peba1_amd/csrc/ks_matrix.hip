// ks_matrix.hip -- the key switch of wide levels as an int8 matrix product on the matrix cores (gfx950).
//
// The key switch is  out = (0, .., 0, b) - sum_{i < kN, j < 8} KSK[i][j][d_ij]  (mod 2^32),  d_ij the j-th base-4 digit of
// a_i + prec_offset (digit j at bits [31 - 2j, 30 - 2j]), a zero digit contributing nothing.  Written as a product:
//
//   A [gates][K]    one-hot, never stored: K = kN * 8 * 4, entry ((i, j), v) is 1 where d_ij = v.  The four K-entries of
//                   (i, j) are the bytes of the single word 1 << (8 d_ij).
//   B [K][columns]  the byte planes of the key (ksk_planes_kernel, once per key): every KSK word w as four signed bytes
//                   s_0 .. s_3 in [-128, 127] with sum_p s_p 2^(8p) = w (mod 2^32) (ks_matrix.hpp ks_byte_planes); row
//                   ((i, j), v) of plane p holds s_p of KSK[i][j][v], the rows of v = 0 are zero.
//   acc_p = A B_p   in i32: a gate has kN * 8 ones in its row, |acc_p| <= kN * 8 * 128 -- 2^20 at N = 1024, 2^21 at 2048.
//   out = (0, b) - sum_p (acc_p << 8p)    in wrapping u32: word for word the sum above.
//
// One v_mfma_i32_32x32x32_i8 covers K = 32: the 8 digits of one coefficient i.  K-order within the instruction: lane L
// holds, of its row (A: gate L % 32) or column (B: output word L % 32), the 16 K-entries 16 h .. 16 h + 15 with h = L / 32,
// register r byte v being K-entry 16 h + 4 r + v -- that is digit j = 4 h + r, value v.  A and B use the same K map, and
// the sum over K does not depend on its order, so the kernel needs only that the two maps agree; the result map is the
// one of every 32x32 MFMA: lane L register r = row 8 (r / 4) + 4 (L / 32) + r % 4, column L % 32
// (tests/test_gpu_ks_matrix.py runs exact integer data with an asymmetric B through it).
//
// Image layout: [column tile of 32 words][i][plane][lane 64] x 16 bytes -- a lane's B operand of one K-step is one 16-byte
// load, a wave's four planes 4 KB contiguous, and the walk over i is a linear stream.  No LDS staging of B.
//
// keyswitch_matrix_kernel: a workgroup takes KSM_GATES gates x one column tile (32 words x 4 planes, all four planes of a
// word in one lane's accumulators).  Its KSM_WAVES waves split the coefficients i; each stages the words a_i of its gates
// through a private LDS block (transposed: [i][gate]), forms the A registers with a shift and a bit-field extract, and
// runs 8 MFMAs per i.  The planes are recombined in registers, the waves' sums added through LDS, and the result goes
// straight to the pool slots: no partial sums in memory, no reduce launch.  The last tile of a level is masked: a gate past
// the end reads no row of its own (its staging loads repeat the tile's first gate's, so that the loads stay unconditional),
// its a_i are staged as 0 without the offset -- every digit 0, the zero rows -- and it writes nothing.
// Workgroups of one column tile are given to one XCD (block b runs on XCD b % 8), so that a tile's stream of the image is
// fetched into one L2.
#include "ks_matrix.hpp"

namespace tfhe_hip {

typedef int ksm_v4 __attribute__((ext_vector_type(4)));
typedef int ksm_v16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void ksk_planes_kernel(DevParams p, DevKey key, uint4 *__restrict__ image, long long total) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int lane = (int)(id & 63), plane = (int)((id >> 6) & 3);
    const long long ti = id >> 8;                        // column tile * nin + i
    const int nin = p.k * p.N;
    const int i = (int)(ti % nin), wt = (int)(ti / nin);
    const int w = wt * KSM_WORDS + (lane & 31), h = lane >> 5;
    uint32_t out[4] = {0u, 0u, 0u, 0u};
    if (w < p.ct_stride) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t row = ((size_t)i * 8 + (size_t)(4 * h + r)) * 3;
#pragma unroll
            for (int v = 1; v < 4; ++v) {
                int8_t s[4];
                ks_byte_planes((uint32_t)key.ksk[(row + (size_t)(v - 1)) * p.ct_stride + w], s);
                out[r] |= (uint32_t)(uint8_t)s[plane] << (8 * v);
            }
        }
    }
    image[id] = make_uint4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(KSM_WAVES * 64) void keyswitch_matrix_kernel(DevParams p, const uint4 *__restrict__ image,
                                                                          const int32_t *__restrict__ u_buf,
                                                                          const KsDesc *__restrict__ descs, int count,
                                                                          int32_t *__restrict__ pool, int tiles, int wtiles, int per) {
    constexpr int MS = KSM_GATES / 32;                   // 32-gate row blocks of the tile
    constexpr int REPS = KSM_GATES / 8;                  // staging: 8 gates x 128 bytes per wave-wide load
    constexpr int BLOCK = KSM_CHUNK * KSM_GATES;         // words of a wave's LDS block: the staged a_i, then the wave's sums
    static_assert(BLOCK == 16 * MS * 64 && KSM_CHUNK == 32 && (16 * MS) % KSM_WAVES == 0, "one LDS block serves both uses");
    __shared__ uint32_t lds[KSM_WAVES * BLOCK];
    const int bid = (int)blockIdx.x, vid = (bid & 7) * per + (bid >> 3);
    if (vid >= tiles * wtiles) return;                   // (the whole workgroup: no barrier is left waiting)
    const int wt = vid / tiles, g0 = (vid - wt * tiles) * KSM_GATES;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nin = p.k * p.N, span = nin / KSM_WAVES, i_lo = wave * span, i_hi = i_lo + span;
    uint32_t *su = lds + wave * BLOCK;
    const int part = lane & 7, h = lane >> 5;

    // rows the staging loads of this lane read: a gate past the end of the level reads the tile's first gate (always inside
    // the level) and is masked to zero; a gate without a second operand reads its first twice and masks that
    int src0[REPS], src1[REPS];
    uint32_t keep0[REPS], keep1[REPS];
    const KsDesc dfirst = descs[g0];
#pragma unroll
    for (int rep = 0; rep < REPS; ++rep) {
        const int g = g0 + rep * 8 + (lane >> 3);
        const KsDesc d = descs[g < count ? g : g0];
        keep0[rep] = g < count ? ~0u : 0u;
        keep1[rep] = g < count && d.u1 >= 0 ? ~0u : 0u;
        src0[rep] = g < count ? d.u0 : dfirst.u0;
        src1[rep] = keep1[rep] ? d.u1 : src0[rep];
    }

    ksm_v16 acc[MS][4];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
#pragma unroll
        for (int pl = 0; pl < 4; ++pl)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ms][pl][r] = 0;

    // the B stream of this column tile: 256 lanes-of-16-bytes per i; a ring of four K-steps, three requested ahead
    const uint4 *bsrc = image + (size_t)wt * (size_t)nin * 256 + lane;
    uint4 b[4][4];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int pl = 0; pl < 4; ++pl) b[s][pl] = bsrc[(size_t)(i_lo + s) * 256 + pl * 64];

    for (int ic = i_lo; ic < i_hi; ic += KSM_CHUNK) {
        // stage a_i + offset of KSM_CHUNK coefficients of every gate, transposed; column g ^ 8 (ii / 4) keeps both the
        // writes (8 gates x 8 parts a load) and the reads (32 gates of one ii) on distinct banks
#pragma unroll
        for (int rep = 0; rep < REPS; ++rep) {
            uint4 v = *reinterpret_cast<const uint4 *>(u_buf + (size_t)src0[rep] * p.u_stride + ic + 4 * part);
            const uint4 v1 = *reinterpret_cast<const uint4 *>(u_buf + (size_t)src1[rep] * p.u_stride + ic + 4 * part);
            const uint32_t off = p.ks_prec_offset;
            v.x = ((v.x + off) & keep0[rep]) + (v1.x & keep1[rep]); v.y = ((v.y + off) & keep0[rep]) + (v1.y & keep1[rep]);
            v.z = ((v.z + off) & keep0[rep]) + (v1.z & keep1[rep]); v.w = ((v.w + off) & keep0[rep]) + (v1.w & keep1[rep]);
            const int col = (rep * 8 + (lane >> 3)) ^ (part << 3);
            su[(4 * part + 0) * KSM_GATES + col] = v.x;
            su[(4 * part + 1) * KSM_GATES + col] = v.y;
            su[(4 * part + 2) * KSM_GATES + col] = v.z;
            su[(4 * part + 3) * KSM_GATES + col] = v.w;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int ii = 0; ii < KSM_CHUNK; ii += 4) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int i = ic + ii + s, inext = i + 3 < i_hi ? i + 3 : i_hi - 1;
#pragma unroll
                for (int pl = 0; pl < 4; ++pl) b[(s + 3) & 3][pl] = bsrc[(size_t)inext * 256 + pl * 64];
                ksm_v4 a[MS];
#pragma unroll
                for (int ms = 0; ms < MS; ++ms) {
                    const uint32_t x = su[(ii + s) * KSM_GATES + ((ms * 32 + (lane & 31)) ^ ((((ii + s) >> 2) & 7) << 3))];
                    const uint32_t y = x >> (24 - 8 * h);                 // digits 4 h .. 4 h + 3, the first on top
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[ms][r] = (int)(1u << (((y >> (6 - 2 * r)) & 3u) << 3));
                }
#pragma unroll
                for (int ms = 0; ms < MS; ++ms)
#pragma unroll
                    for (int pl = 0; pl < 4; ++pl) {
                        const uint4 bw = b[s][pl];
                        const ksm_v4 bv = {(int)bw.x, (int)bw.y, (int)bw.z, (int)bw.w};
                        acc[ms][pl] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[ms], bv, acc[ms][pl], 0, 0, 0);
                    }
                // (keeps each step's requests in its own step: the scheduler would otherwise issue four steps' loads in one
                // burst and wait for all of them at the next step)
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }

    // the planes of a word back into the word, then the waves' sums through LDS; wave q finishes a share of the registers
    uint32_t o[16 * MS];
#pragma unroll
    for (int ms = 0; ms < MS; ++ms)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            o[ms * 16 + r] = (uint32_t)acc[ms][0][r] + ((uint32_t)acc[ms][1][r] << 8) + ((uint32_t)acc[ms][2][r] << 16) +
                             ((uint32_t)acc[ms][3][r] << 24);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 16 * MS; ++q) su[q * 64 + lane] = o[q];
    __syncthreads();
    constexpr int SHARE = 16 * MS / KSM_WAVES;
    const int w = wt * KSM_WORDS + (lane & 31);
#pragma unroll
    for (int e = 0; e < SHARE; ++e) {
        const int q = wave * SHARE + e;
        uint32_t sum = 0;
#pragma unroll
        for (int v = 0; v < KSM_WAVES; ++v) sum += lds[v * BLOCK + q * 64 + lane];
        const int r = q & 15, g = g0 + (q >> 4) * 32 + 8 * (r >> 2) + 4 * h + (r & 3);
        if (g >= count || w >= p.ct_stride) continue;
        const KsDesc d = descs[g];
        uint32_t val = 0u - sum;
        if (w == p.n) {
            val += (uint32_t)u_buf[(size_t)d.u0 * p.u_stride + nin] + (uint32_t)d.add_b;
            if (d.u1 >= 0) val += (uint32_t)u_buf[(size_t)d.u1 * p.u_stride + nin];
        }
        if (w > p.n) val = 0u;
        pool[(size_t)d.dst_slot * p.ct_stride + w] = (int32_t)val;
    }
}

bool launch_ksk_planes(hipStream_t s, const DevParams &p, const DevKey &key, uint8_t *image) {
    const int nin = p.k * p.N;
    if (!image || !ks_matrix_shape_ok(nin, p.ks_t, p.ks_basebit)) return false;
    const long long total = (long long)(ks_matrix_image_bytes(nin, p.ct_stride) / 16);
    hipLaunchKernelGGL(ksk_planes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p, key,
                       reinterpret_cast<uint4 *>(image), total);
    return true;
}

bool launch_keyswitch_matrix(hipStream_t s, const DevParams &p, const uint8_t *image, const int32_t *u_buf,
                             const KsDesc *descs, int count, int32_t *pool) {
    const int nin = p.k * p.N;
    if (!image || count <= 0 || !ks_matrix_shape_ok(nin, p.ks_t, p.ks_basebit) || (p.u_stride & 3)) return false;
    const long long tiles = (count + KSM_GATES - 1) / KSM_GATES, wtiles = (p.ct_stride + KSM_WORDS - 1) / KSM_WORDS;
    const long long per = (tiles * wtiles + 7) / 8;
    if (per * 8 > 0x7fffffffLL) return false;
    hipLaunchKernelGGL(keyswitch_matrix_kernel, dim3((unsigned)(per * 8)), dim3(KSM_WAVES * 64), 0, s, p,
                       reinterpret_cast<const uint4 *>(image), u_buf, descs, count, pool, (int)tiles, (int)wtiles, (int)per);
    return true;
}

}  // namespace tfhe_hip
