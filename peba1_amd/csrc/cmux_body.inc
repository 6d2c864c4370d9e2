// cmux_body.inc -- the one body of the kernels of cmux.hip, included into each of them as text (as br8_body.inc is into the
// blind rotations): cmux_kernel<., false>, cmux_kernel<., true> and inner_kernel compile exactly the statements below, and
// the first two exactly the instructions they had before there was a third.  The including kernel provides
//   LOGN                  the template parameter
//   MODE                  constexpr int: MODE_CMUX (d1 - d0), MODE_ROT (X^(-rot) d0 - d0), MODE_PRODUCT (d0 itself, nothing added)
//   a                     the CmuxArgs
//   t                     the RingRows (looked at under MODE_PRODUCT alone)
    constexpr bool ROT = MODE == MODE_ROT;
    using NTT = WaveNtt<LOGN>;
    constexpr int N = NTT::N, REGS = NTT::REGS;
    __shared__ __align__(16) uint32_t lds_scr[2][NTT::SCRATCH_WORDS];
    // residues in natural order, [prime = the wave that wrote them][output polynomial][N]
    __shared__ __align__(16) uint32_t lds_x[2][2][N];
    const int tid = threadIdx.x;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const PrimeCtx c = ring_prime_ctx(q, a.tw, N);
    uint32_t *scr = lds_scr[q];

    const int cm = blockIdx.x;                                   // < a.count: the grid is a.count workgroups
    const int32_t *d0 = a.d0 + (size_t)cm * a.stride;
    const bool has_d1 = cm < a.n_d1;                             // workgroup-uniform
    const int32_t *d1 = a.d1 + (size_t)cm * a.stride;            // read only if has_d1
    const uint32_t mask = (1u << a.Bgbit) - 1u;
    const int32_t half = 1 << (a.Bgbit - 1);
    typename NTT::FwdTw0 t0;                 // lane-uniform and the same for every transform
    t0.load(c, lane);

    int64_t acc0[REGS], acc1[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) { acc0[r] = 0; acc1[r] = 0; }
    // image of row (bit, u, p): [X = bit (k+1) l + u l + p][prime][polynomial 2][N] (kernels.hip bk_transform_kernel, nw = 2)
    const uint4 *rowimg = reinterpret_cast<const uint4 *>(a.img + ((size_t)a.bit * 2 * a.l * 2 + q) * 2 * N) + lane;
    for (int u = 0; u < 2; ++u) {
        // coefficient j = 64 r + lane of polynomial u (layout L0 of ntt_wave.hpp)
        uint32_t v[REGS];
#pragma unroll
        for (int r = 0; r < REGS; ++r) {
            const int j = u * N + r * 64 + lane;
            if constexpr (ROT) {
                // (X^(-rot) d0)[j] = d0[j + rot], and -d0[j + rot - N] past the wrap (lut_coef's convention); 0 < rot < N
                const int jr = r * 64 + lane + a.rot;
                const uint32_t w = (uint32_t)d0[u * N + (jr & (N - 1))];
                v[r] = (jr >= N ? 0u - w : w) - (uint32_t)d0[j] + a.offset;
            } else if constexpr (MODE == MODE_PRODUCT) {
                v[r] = (uint32_t)d0[j] + a.offset;
            } else {
                v[r] = (has_d1 ? (uint32_t)d1[j] : 0u) - (uint32_t)d0[j] + a.offset;
            }
        }
        for (int p = 0; p < a.l; ++p) {
            const int shift = 32 - (p + 1) * a.Bgbit;
            int32_t x[REGS];
#pragma unroll
            for (int r = 0; r < REGS; ++r) x[r] = (int32_t)((v[r] >> shift) & mask) - half;    // |x| <= Bg/2 <= 2^11
            NTT::template forward<false>(x, c, scr, lane, t0);            // |x| < 6.1 P / 6.7 P (cmux.hpp)
            const uint4 *bp = rowimg + (size_t)(u * a.l + p) * N;       // 4N words per row = N uint4
#pragma unroll
            for (int g = 0; g < REGS / 4; ++g) {
                const uint4 b0 = bp[g * 64], b1 = bp[N / 4 + g * 64];
                acc0[4 * g + 0] += (int64_t)x[4 * g + 0] * (int32_t)b0.x;
                acc0[4 * g + 1] += (int64_t)x[4 * g + 1] * (int32_t)b0.y;
                acc0[4 * g + 2] += (int64_t)x[4 * g + 2] * (int32_t)b0.z;
                acc0[4 * g + 3] += (int64_t)x[4 * g + 3] * (int32_t)b0.w;
                acc1[4 * g + 0] += (int64_t)x[4 * g + 0] * (int32_t)b1.x;
                acc1[4 * g + 1] += (int64_t)x[4 * g + 1] * (int32_t)b1.y;
                acc1[4 * g + 2] += (int64_t)x[4 * g + 2] * (int32_t)b1.z;
                acc1[4 * g + 3] += (int64_t)x[4 * g + 3] * (int32_t)b1.w;
            }
        }
    }
    // |acc| < (k+1) l f P^2 -> reduction below 4 P (MAC bound) -> inverse NTT: signed residues below P, natural order
    int32_t y[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) y[r] = mont_redc(acc0[r], c.P, c.pinv);
    NTT::inverse(y, c, scr, lane);
#pragma unroll
    for (int r = 0; r < REGS; ++r) lds_x[q][0][r * 64 + lane] = (uint32_t)y[r];
#pragma unroll
    for (int r = 0; r < REGS; ++r) y[r] = mont_redc(acc1[r], c.P, c.pinv);
    NTT::inverse(y, c, scr, lane);
#pragma unroll
    for (int r = 0; r < REGS; ++r) lds_x[q][1][r * 64 + lane] = (uint32_t)y[r];
    // the waves took different primes and now exchange through LDS alone: the barrier form ntt_wave.hpp documents for
    // that (both waves reach it on the same path; nothing was stored to global memory yet)
    lds_barrier();
    if constexpr (MODE == MODE_PRODUCT) {
        ring_crt_rows<LOGN>(lds_x, q, lane, tid, cm, a.out, t);    // the CRT, the full product, the rows (ring_wave.hpp)
        return;
    }
    // wave q owns output polynomial q: coefficients 4 (64 g + lane) .. + 3, both primes' residues, the signed CRT
    // (the true integer is below CRT_EXACT_LIMIT: CRT bound), + d0, one 16-byte store
    const uint4 *r0 = reinterpret_cast<const uint4 *>(lds_x[0][q]) + lane;
    const uint4 *r1 = reinterpret_cast<const uint4 *>(lds_x[1][q]) + lane;
    const uint4 *src = reinterpret_cast<const uint4 *>(d0 + (size_t)q * N) + lane;
    uint4 *dst = reinterpret_cast<uint4 *>(a.out + ((size_t)cm * 2 + q) * N) + lane;
#pragma unroll
    for (int g = 0; g < REGS / 4; ++g) {
        const uint4 x0 = r0[g * 64], x1 = r1[g * 64], base = src[g * 64];
        dst[g * 64] = make_uint4(base.x + crt_signed_to_torus((int32_t)x0.x, (int32_t)x1.x),
                                 base.y + crt_signed_to_torus((int32_t)x0.y, (int32_t)x1.y),
                                 base.z + crt_signed_to_torus((int32_t)x0.z, (int32_t)x1.z),
                                 base.w + crt_signed_to_torus((int32_t)x0.w, (int32_t)x1.w));
    }
