// rtfhe_body_wg.hpp -- the body of k_bootstrap_wg and of its programmable-bootstrap twin k_pbs_wg (rtfhe_kernels_wg.hpp), included inside the braces of both
// kernels: they declare `a` (the family's arguments) and `tvs` (where the accumulator starts and how the step decomposes: TvGate / TvLut / TvMany / TvEnc / TvManyR / TvEncR, rtfhe_kernels.hpp).
// The body is text, not a __device__ function, so that k_bootstrap_wg compiles to exactly what it did before the twin existed
// (a function taking the arguments by reference changes instruction order and scalar registers).  No include guard: included five times (k_pbs_many_*: the many-LUT PBS; k_pbs_enc_*: encrypted tables; k_pbs_round_*: both with the rounded decomposition).
    typedef Geo<LOGN> G;
    typedef WgLds<LOGN, L> S;
    constexpr int N = G::N, P = G::P, R = G::R, NW = S::NW, ROWS = 2 * L;
    static_assert(R == NW, "the MAC phase gives each of the 8 waves one of the R = 8 points a lane holds");
    static_assert(ROWS + 2 == NW, "rows 0..2l-1 start on waves 0..2l-1; the last two rows finish on waves 2l, 2l+1");
    constexpr uint32_t MA = decomp_add(L, BGBIT, decltype(tvs)::ROUNDED), MX = decomp_xor(L, BGBIT, decltype(tvs)::ROUNDED);
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem + S::TW);
    uint32_t* accbuf = reinterpret_cast<uint32_t*>(smem + S::ACC);
    cplx* spec = reinterpret_cast<cplx*>(smem + S::SPEC);
    cplx* sbuf = reinterpret_cast<cplx*>(smem + S::SBUF);
    uint32_t* abar = reinterpret_cast<uint32_t*>(smem + S::ABAR);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const cplx* twf = tw;
    const int g = blockIdx.x;                       // grid = count
    const int n = a.n;

    for (int idx = tid; idx < G::TW_TOTAL; idx += 64 * NW) tw[idx] = a.tw[idx];
    const GateIo io = gate_io(a, g);
    const auto tv = tv_row(tvs, g, N);
    if (!io.ok || !tv.ok()) return;                            // the whole workgroup serves this gate: uniform exit
    {   // pre-step + mod switch (tfhe.rs:41-71, 97, 107-108)
        constexpr int SH = 32 - LOGN - 1;
        for (int i = tid; i <= n; i += 64 * NW) {
            const uint32_t t = gate_linear(io.op, io.p0[i], io.p1[i], i == n);
            if constexpr (decltype(tvs)::MANY) abar[i] = mod_switch<SH>(t, i == n, tv_shift(tvs));   // many-LUT: at SH + t, scaled back
            else abar[i] = (i == n) ? (t >> SH) : ((t + (1u << (SH - 1))) >> SH);
        }
    }
    __syncthreads();
    {   // acc = X^{-bbar} * testvec (tfhe.rs:85, 98-106)
        const int bbar = (int)abar[n];
        for (int c = tid; c < N; c += 64 * NW) {
            const int e = (c + bbar) & (2 * N - 1);
            accbuf[c] = tv_word<LOGN>(tv, e);
            if constexpr (decltype(tvs)::ENC) accbuf[N + c] = tv_word_a<LOGN>(tv, e);   // encrypted table: the a half from the row's a polynomial
            else accbuf[N + c] = 0u;
        }
    }
    __syncthreads();

#ifdef RTFHE_WG_STAMPS
    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = __builtin_amdgcn_s_memtime();
#define WG_STAMP(k) do { unsigned long long t_ = __builtin_amdgcn_s_memtime(); tsum[k] += t_ - tprev; tprev = t_; } while (0)
#else
#define WG_STAMP(k) do { } while (0)
#endif
    const size_t trgsw_cplx = (size_t)ROWS * 2 * R * 64;
    // BK values this wave needs in the M phase: point m = wave of every row and component (coalesced 1 KiB each).
    // Software-pipelined: the values of step i + 1 are requested at the start of step i's I phase (6 of the 8 waves idle
    // there) and have landed by the barrier that ends it.
    cplx bkv[ROWS][2];
    // through a buffer resource: scalar offset of (step, row, component, wave) + one per-lane VGPR (see k_bootstrap_pair)
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t bk_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<cplx*>(a.bk), 0, 0x7fffffff, 0x00020000);
    const int lane16 = lane * 16;
    auto load_bk = [&](int step, cplx (&dst)[ROWS][2]) {
        const int s0 = __builtin_amdgcn_readfirstlane((int)(((size_t)step * trgsw_cplx + (size_t)wave * 64) * sizeof(cplx)));
#pragma unroll
        for (int j = 0; j < ROWS; j++) {
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const v4u v = __builtin_amdgcn_raw_buffer_load_b128(bk_rsrc, lane16, s0 + (j * 2 + c) * R * 64 * (int)sizeof(cplx), 0);
                dst[j][c] = make_double2(__longlong_as_double(((unsigned long long)v.y << 32) | v.x), __longlong_as_double(((unsigned long long)v.w << 32) | v.z));
            }
        }
    };
    if (a.steps > 0) load_bk(0, bkv);
    // waves 0..3 = (component wave >> 1, parity wave & 1) of the I phase: their 15 twiddles stay in registers over the whole blind rotation
    // (the parity tables ride behind the table staged into LDS above)
    Q4Regs qinv;
    qinv.load(a.tw + G::TW_TOTAL + Q4Tw::off(wave >= 4 ? 0 : 1, wave & 1), lane);      // waves 4..7: the forward tables of their half row
#pragma unroll 1
    for (int i = 0; i < a.steps; i++) {
        const int r = __builtin_amdgcn_readfirstlane((int)abar[i]);
        WG_STAMP(0);
        // ---- F: one digit polynomial per row (trgsw.rs:269-289).  Six transforms on four SIMDs: rows 0..3 run whole on waves 0..3 (one per SIMD);
        // rows 4, 5 on waves 4..7 = (row, parity of the point index), one beside every whole-row wave (rtfhe_sub256.hpp).
        if (wave < ROWS - 2) {
            const int h = wave / L, jj = wave - h * L;
            const uint32_t* poly = accbuf + h * N;
            double re[R], im[R];
#pragma unroll
            for (int m = 0; m < R; m++) {
                const int c0 = lane + 64 * m, c1 = c0 + P;
                const uint32_t d0 = rotated_coef<LOGN>(poly, c0, r) - poly[c0];
                const uint32_t d1 = rotated_coef<LOGN>(poly, c1, r) - poly[c1];
                re[m] = (double)decomp_digit((d0 + MA) ^ MX, BGBIT, jj);
                im[m] = (double)decomp_digit((d1 + MA) ^ MX, BGBIT, jj);
            }
            // exchange buffer = this row's own (still unwritten) spectrum slot, one 16-byte access per complex value
            fft_forward<LOGN, 2, BOOT_TRIV>(re, im, twf, reinterpret_cast<double*>(spec + (size_t)wave * S::SROW), lane);
            cplx* dst = spec + (size_t)wave * S::SROW + lane;
#pragma unroll
            for (int m = 0; m < R; m++) dst[m * 64] = make_double2(re[m], im[m]);
        } else {
            // rows 2l-2, 2l-1: wave = (row, parity H); this wave's points are i = 2 (lane + 64 m) + H.  Its half spectrum out_H[j], j = 4 lane + m, goes to
            // words [256 H, 256 H + 256) of the row's slot, index m * 64 + lane; the M phase adds / subtracts the two halves as it reads them.
            const int k = wave - (ROWS - 2), row = (ROWS - 2) + (k >> 1);
            const int h = row / L, jj = row - h * L;
            const uint32_t* poly = accbuf + h * N;
            cplx* half = spec + (size_t)row * S::SROW + (k & 1) * (P / 2);
            cplx* xc = reinterpret_cast<cplx*>(smem + S::XBUF) + (size_t)k * Q4::XS;
            __builtin_amdgcn_s_setprio(0);
            auto run = [&](auto odd) {
                constexpr bool ODD = decltype(odd)::value;
                double re[4], im[4];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int c0 = 2 * (lane + 64 * m) + (ODD ? 1 : 0), c1 = c0 + P;
                    const uint32_t d0 = rotated_coef<LOGN>(poly, c0, r) - poly[c0];
                    const uint32_t d1 = rotated_coef<LOGN>(poly, c1, r) - poly[c1];
                    re[m] = (double)decomp_digit((d0 + MA) ^ MX, BGBIT, jj);
                    im[m] = (double)decomp_digit((d1 + MA) ^ MX, BGBIT, jj);
                }
                sub256_forward<ODD, BOOT_TRIV>(re, im, qinv, xc, lane, [](int k) { if (k == 2) __builtin_amdgcn_s_setprio(1); });
#pragma unroll
                for (int m = 0; m < 4; m++) half[m * 64 + lane] = make_double2(re[m], im[m]);
            };
            if (k & 1) run(std::true_type{}); else run(std::false_type{});
            __builtin_amdgcn_s_setprio(0);
        }
        WG_STAMP(1);
        __syncthreads();
        WG_STAMP(2);
        // ---- M: hadamard + fold-add from zero in row order (spqlios.rs:204-222, trgsw.rs:290-299), point m = wave ----
        {
            double s0r = 0.0, s0i = 0.0, s1r = 0.0, s1i = 0.0;
            const cplx* src = spec + wave * 64 + lane;
#pragma unroll
            for (int j = 0; j < ROWS; j++) {
                cplx d;
                if (j < ROWS - 2) d = src[(size_t)j * S::SROW];
                else {      // point 8 lane + wave = 2 jq + (wave & 1), jq = 4 lane + (wave >> 1): out_0[jq] + out_1[jq] or out_0[jq] + (-out_1[jq])
                    const cplx* hs = spec + (size_t)j * S::SROW + (wave >> 1) * 64 + lane;
                    const cplx e = hs[0], o = hs[P / 2];
                    d = (wave & 1) ? make_double2(e.x + (-o.x), e.y + (-o.y)) : make_double2(e.x + o.x, e.y + o.y);
                }
                {
                    const double ii = bkv[j][0].y * d.y, rr = bkv[j][0].x * d.x, ri = bkv[j][0].x * d.y, ir = bkv[j][0].y * d.x;
                    s0r = s0r + (rr - ii);
                    s0i = s0i + (ir + ri);
                }
                {
                    const double ii = bkv[j][1].y * d.y, rr = bkv[j][1].x * d.x, ri = bkv[j][1].x * d.y, ir = bkv[j][1].y * d.x;
                    s1r = s1r + (rr - ii);
                    s1i = s1i + (ir + ri);
                }
            }
            sbuf[wave * 64 + lane] = make_double2(s0r, s0i);
            sbuf[P + wave * 64 + lane] = make_double2(s1r, s1i);
        }
        WG_STAMP(3);
        __syncthreads();
        WG_STAMP(4);
        cplx bkn[ROWS][2];
        load_bk(i + 1 < a.steps ? i + 1 : i, bkn);
        // ---- I: each component's inverse transform (math.rs:279-288) on two waves, one per parity of the point index; += (trlwe.rs:49-60) ----
        // A lane reads the eight sums s[8 lane .. 8 lane + 7] its parity's four inputs need (both parities read the same words): the size-2 stage
        // across the parities is computed here, in_0[j] = s[2j] + s[2j + 1], in_1[j] = s[2j] + (-s[2j + 1]), j = 4 lane + m -- no trade between the waves.
        if (wave < 4) {
            const int comp = wave >> 1;
            const cplx* src = sbuf + (size_t)comp * P + lane;
            cplx v[R];
#pragma unroll
            for (int m = 0; m < R; m++) v[m] = src[m * 64];
            // the spectra are dead after the M phase: slot `wave` holds this wave's exchange buffers
            cplx* xc = spec + (size_t)wave * S::SROW;
            uint32_t* poly = accbuf + comp * N;
            auto run = [&](auto odd) {
                constexpr bool ODD = decltype(odd)::value;
                double re[4], im[4];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    re[m] = ODD ? v[2 * m].x + (-v[2 * m + 1].x) : v[2 * m].x + v[2 * m + 1].x;
                    im[m] = ODD ? v[2 * m].y + (-v[2 * m + 1].y) : v[2 * m].y + v[2 * m + 1].y;
                }
                sub256_inverse<ODD, BOOT_TRIV>(re, im, qinv, xc, lane);
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const int c = 2 * (lane + 64 * m) + (ODD ? 1 : 0);
                    poly[c] += trunc_to_torus(re[m]);
                    poly[c + P] += trunc_to_torus(im[m]);
                }
            };
            if (wave & 1) run(std::true_type{}); else run(std::false_type{});
        }
        WG_STAMP(5);
        __syncthreads();
        WG_STAMP(6);
#pragma unroll
        for (int j = 0; j < ROWS; j++) { bkv[j][0] = bkn[j][0]; bkv[j][1] = bkn[j][1]; }
    }
#ifdef RTFHE_WG_STAMPS
    if (a.dbg && blockIdx.x == 0 && lane == 0)
        for (int k = 0; k < 8; k++) a.dbg[wave * 8 + k] = tsum[k];
#endif

    if (a.mode == MODE_BLIND_ROTATE) {
        uint32_t* o = a.out + (size_t)g * 2 * N;
        for (int c = tid; c < 2 * N; c += 64 * NW) o[c] = accbuf[c];
        return;
    }

    // sample extract index 0 (trlwe.rs:110-121) into the now free abar/spec area is not needed: a' is written over a(X)
    uint32_t av[N / (64 * NW)];
#pragma unroll
    for (int k = 0; k < N / (64 * NW); k++) av[k] = accbuf[N + tid + 64 * NW * k];
    const uint32_t bprime = accbuf[0];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N / (64 * NW); k++) {
        const int c = tid + 64 * NW * k;
        accbuf[N + ((N - c) & (N - 1))] = (c == 0) ? av[k] : (0u - av[k]);
    }
    __syncthreads();
    if constexpr (decltype(tvs)::MANY) {      // many-LUT PBS (MODE_EXTRACT only): every output (the batch key switch writes the output rows)
        many_extract<N>(a.ext, a.ext_first + g, tv_shift(tvs), accbuf, tid, N, 64 * NW, tid);
        return;
    }
    if (a.mode == MODE_EXTRACT) {      // the key switch of the whole batch follows as its own launch (k_key_switch_mm)
        const int ge = a.ext_first + g;      // batch-wide gate number: the sample buffer is laid out for the key switch (ext_slot)
        for (int c = tid; c < N; c += 64 * NW) *ext_slot(a.ext, ge, c, N) = accbuf[N + c];
        if (tid == 0) *ext_slot(a.ext, ge, N, N) = bprime;
        for (int c = tid; c <= n; c += 64 * NW) io.out[c] = 0u;
        return;
    }
    // key switch: wave w sums the rows of coefficients [w N/8, (w+1) N/8); partial sums meet in LDS
    uint4 sum[KSQ];
    ks_accumulate<LOGN, KS_T, KS_BB, KSQ>(accbuf + N, wave * (N / NW), (wave + 1) * (N / NW), a.ksk, a.ksw, sum, lane);
    uint4* part = reinterpret_cast<uint4*>(spec);          // [NW][KSQ][64] uint4 = 24 KiB
#pragma unroll
    for (int q = 0; q < KSQ; q++) part[(wave * KSQ + q) * 64 + lane] = sum[q];
    __syncthreads();
    uint32_t* out = io.out;
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(spec);
    for (int col = tid; col <= n; col += 64 * NW) {
        // column col lives in uint4 slot (col/4) = lane + 64 q, element col % 4
        const int slot = col >> 2, q = slot >> 6, ln = slot & 63, e = col & 3;
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) s += pw[((w * KSQ + q) * 64 + ln) * 4 + e];
        out[col] = ((col == n) ? bprime : 0u) - s;
    }
