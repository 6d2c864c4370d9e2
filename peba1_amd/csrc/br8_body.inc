// br8_body.inc -- the body of the 8-wave blind-rotate kernel (kernels.hip), included by blind_rotate8_kernel and by its
// multi-key form blind_rotate8_mk_kernel.  Textual inclusion keeps the single-key kernel's code exactly what it was when
// the body was written in place (the same body as an inlined function compiles to a different register allocation).
// Expects in scope: LOGN, TAB, p, key, pool, rots, u_buf, acc_dbg, sh; BR8_TAG (0 single-key, 1 multi-key) tags the
// forward_poly instantiation so that each kernel has a row function of its own.
    using NTT = WaveNtt<LOGN>;
    using SUB = WaveNtt<LOGN - 1>;
    constexpr int N = NTT::N, M = N / 2, REGS = NTT::REGS, RS = SUB::REGS, QUARTER = RS / 4;
    const int tid = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int base = wv & 3, q = base & 1, u = base >> 1;
    const bool role_b = wv >= 4;
    const int h = wv >> 2;                              // the half of every inverse transform this wave runs
    const int lane = tid & 63;
    PrimeCtx c = make_ctx(q, key.tw, N);
    const PrimeCtx ch = make_sub_ctx(q, h, key.tw, N);  // twiddles of half h (engine.cpp make_twiddles)
    const uint32_t iw1_0 = key.tw[(size_t)1 * N + 1], iw1_1 = key.tw[(size_t)3 * N + 1];   // inverse stage 0, both primes
    uint32_t *scr = sh.scr[wv];
    const int n = p.n;
    const RotDesc rd = rots[blockIdx.x];
    ClockProbe clk;
    clk.begin(p);

    prelude_modswitch<LOGN, 512>(p, rd, pool, sh.bar, tid);
    if constexpr (TAB) {
        // the four waves of prime q fill that prime's table
        NTT::build_digit_table(sh.dtab[q], c, p.Bgbit, ((wv >> 1) << 6) | lane, 256);
        c.dtab = sh.dtab[q];
    }
    if (wv < 2) {                                    // waves 0 and 1 = (q, u = 0, A): prime q's twiddles into LDS, once
        typename NTT::FwdTw1 a;
        a.load(c, lane);
        if ((lane & ((1 << NTT::LC) - 1)) == 0) a.to_image(sh.ft1[q][lane >> NTT::LC]);
        typename NTT::FwdTw2 b;
        b.load(c, lane);
        b.to_image(sh.ft2[q][lane]);
    }
    c.fw1 = sh.ft1[q][lane >> NTT::LC];
    c.fw2 = sh.ft2[q][lane];
    __syncthreads();
    if (q == 0 && !role_b) {
        const int barb = sh.bar[n];
        const int32_t *lut = lut_of(p, rd);
#pragma unroll
        for (int r = 0; r < REGS; ++r) {
            const int j = r * 64 + lane;
            sh.acc.set(u, j, u == 0 ? 0u : body_coef<LOGN>(lut, j, barb, p.mu));
        }
    }
    __syncthreads();

    // (Round 5 built the balanced assignment -- rows [0, l/2) to A, [(l+1)/2, l) to B, the middle row of an odd l shared: A its
    // transform's first pass, B the rest, 940 / 1,010 vector instructions per step instead of 1,144 / 764 -- and measured it
    // SLOWER, 3.21 against 2.82 ms per rotation: the two waves of a SIMD are arbitrated by age, the older wave A runs at the
    // pace of a lone wave and B fills its bubbles, which 764 instructions just about do; a balanced pair leaves B to finish
    // alone.  profiles/r05_ab_kernel_variants.txt; DESIGN.md section 5.)
    const int last = p.l - 1;
    typename NTT::FwdTw0 t0;
    t0.load(c, lane);
    STAMP_DECL;
    // wave A -- the older wave of its SIMD and the one with more work -- also holds the higher issue priority for the whole
    // rotation: explicit priority instead of age alone measured 2.74 against 2.77 ms per rotation, 3.18 against 3.24 ms per
    // 256 (profiles/r05_ab_kernel_variants.txt); dropping it for the step's tail: 2.88
    if (!role_b) __builtin_amdgcn_s_setprio(1);
    for (int i = 0; i < n; ++i) {
        const int abar = __builtin_amdgcn_readfirstlane((int)sh.bar[i]);
        if (abar == 0) continue;
        STAMP(0);
        {
            int64_t acc0[REGS], acc1[REGS];             // output poly u, output poly 1-u
            if (!role_b)
                forward_poly<LOGN, true, TAB, true, false, BR8_TAG>(p, key, c, sh.acc, scr, lane, q, i, u, abar, u != 0,
                                                                                acc0, acc1, t0, 0, last);
            else
                forward_poly<LOGN, true, TAB, true, false, BR8_TAG>(p, key, c, sh.acc, scr, lane, q, i, u, abar, u != 0,
                                                                                acc0, acc1, t0, last, last + 1);
            STAMP(1);
            int32_t s0[REGS], s1[REGS];
#pragma unroll
            for (int r = 0; r < REGS; ++r) {
                s0[r] = mont_redc(acc0[r], c.P, c.pinv);                // at most l-1 rows: |.| < 0.93P
                s1[r] = mont_redc(acc1[r], c.P, c.pinv);
            }
            NTT::write_row(s0, role_b ? sh.pb0[base] : sh.pa0[base], lane);
            NTT::write_row(s1, role_b ? sh.pb[base] : sh.pa1[base], lane);
        }
        typename SUB::InvTw2 t2;                            // requested before the barrier, in flight across it
        t2.load(ch, lane);
        STAMP(2);
        lds_barrier();
        STAMP(3);
        {
            // Half h of the summed spectrum of output polynomial u, in the half transform's layout: slot 8 lane + reg of
            // the half is slot 16 (32 h + lane / 2) + 8 (lane & 1) + reg of the full-size rows the forward phase wrote
            const int off = NTT::row_base(32 * h + (lane >> 1)) + RS * (lane & 1);
            const uint32_t *rows[4] = {sh.pa0[base] + off, sh.pb0[base] + off, sh.pa1[base ^ 2] + off, sh.pb[base ^ 2] + off};
            int32_t t[RS];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int g = 0; g < RS / 4; ++g) {
                    const uint4 v = reinterpret_cast<const uint4 *>(rows[k])[g];
                    if (k == 0) { t[4 * g] = (int32_t)v.x; t[4 * g + 1] = (int32_t)v.y; t[4 * g + 2] = (int32_t)v.z; t[4 * g + 3] = (int32_t)v.w; }
                    else { t[4 * g] += (int32_t)v.x; t[4 * g + 1] += (int32_t)v.y; t[4 * g + 2] += (int32_t)v.z; t[4 * g + 3] += (int32_t)v.w; }
                }
            }                                                           // |.| < 3.3P (the inverse takes < 4P)
            // (layout R for this inverse: measured, round 4 -- with layout H the compiler's schedule of this kernel came out
            // 0.13 ms per rotation slower, 2.87 against 2.74 ms, although H saves LDS cycles here too; profiles/archive/r04_ab_*.txt)
            SUB::template inverse<false>(t, ch, scr, lane, t2);      // half-transform outputs, natural order, |t| < P
#pragma unroll
            for (int r = 0; r < RS; ++r) scr[r * 64 + lane] = (uint32_t)t[r];
        }
        STAMP(4);
        lds_barrier();
        STAMP(5);
        {
            // the four waves of output polynomial u take a quarter of the register rows each and finish coefficients
            // j and j + N/2 of it, for both primes (split_finish: last inverse stage, CRT)
            const uint32_t *a0 = sh.scr[(u << 1)], *a1 = sh.scr[(u << 1) | 4];
            const uint32_t *b0 = sh.scr[(u << 1) | 1], *b1 = sh.scr[(u << 1) | 5];
            const int part = q | (h << 1);
#pragma unroll
            for (int r = 0; r < QUARTER; ++r) {
                const int jl = (part * QUARTER + r) * 64 + lane;
                const int32_t va0 = (int32_t)a0[jl], va1 = (int32_t)a1[jl], vb0 = (int32_t)b0[jl], vb1 = (int32_t)b1[jl];
                sh.acc.set(u, jl, sh.acc.get(u, jl) + split_finish(0, va0, va1, vb0, vb1, iw1_0, iw1_1));
                sh.acc.set(u, M + jl, sh.acc.get(u, M + jl) + split_finish(1, va0, va1, vb0, vb1, iw1_0, iw1_1));
            }
        }
        STAMP(6);
        lds_barrier();
        STAMP(7);
    }
    STAMP_FLUSH;
    extract_sample<LOGN, 512>(p, rd, sh.acc, u_buf, acc_dbg, tid);
    clk.end(p);
