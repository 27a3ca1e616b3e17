// rtfhe_body_wave.hpp -- the body of k_bootstrap and of its programmable-bootstrap twin k_pbs (rtfhe_kernels.hpp), included inside the braces of both
// kernels: they declare `a` (the family's arguments) and `tvs` (where the accumulator starts and how the step decomposes: TvGate / TvLut / TvMany / TvEnc / TvManyR / TvEncR, rtfhe_kernels.hpp).
// The body is text, not a __device__ function, so that k_bootstrap compiles to exactly what it did before the twin existed
// (a function taking the arguments by reference changes instruction order and scalar registers).  No include guard: included five times (k_pbs_many_*: the many-LUT PBS; k_pbs_enc_*: encrypted tables; k_pbs_round_*: both with the rounded decomposition).
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = reinterpret_cast<cplx*>(smem);
    TwStage<LOGN>::stage(tw, a.tw, tid, 64 * WAVES);
    __syncthreads();
    // from here on waves never synchronise with each other

    const int g = blockIdx.x * WAVES + wave;
    if (g >= a.count) return;

    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    unsigned char* wbase = smem + (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)wave * bootstrap_wave_lds_bytes<LOGN>(a.npad, DUAL);
    double* xbuf = reinterpret_cast<double*>(wbase);
    uint32_t* accbuf = reinterpret_cast<uint32_t*>(wbase + (size_t)G::XSLOTS * sizeof(double) * (DUAL ? 2 : 1));
    uint32_t* abar = accbuf + 2 * N;
    const cplx* twf = TwStage<LOGN>::fwd(tw);
    const cplx* twi = TwStage<LOGN>::inv_small(tw);
    const cplx* twi_big = TwStage<LOGN>::inv_big(tw, a.tw);

    const int n = a.n;
    // pre-step + mod switch (tfhe.rs:97, 107-108): b floor, a_i rounded, both to [0, 2N)
    const GateIo io = gate_io(a, g);
    const auto tv = tv_row(tvs, g, N);
    if (!io.ok || !tv.ok()) return;
    {
        constexpr int SH = 32 - LOGN - 1;
        for (int i = lane; i <= n; i += 64) {
            const uint32_t t = gate_linear(io.op, io.p0[i], io.p1[i], i == n);
            if constexpr (decltype(tvs)::MANY) abar[i] = mod_switch<SH>(t, i == n, tv_shift(tvs));   // many-LUT: at SH + t, scaled back
            else abar[i] = (i == n) ? (t >> SH) : ((t + (1u << (SH - 1))) >> SH);
        }
    }
    wave_lds_sync();
    // acc = X^{-bbar} * testvec, gates: testvec = (1/8, ..., 1/8 ; 0)   (tfhe.rs:85, 98-106)
    {
        const int bbar = (int)abar[n];
#pragma unroll
        for (int mm = 0; mm < 2 * R; mm++) {
            const int c = lane + 64 * mm;
            const int e = (c + bbar) & (2 * N - 1);
            accbuf[c] = tv_word<LOGN>(tv, e);
            if constexpr (decltype(tvs)::ENC) accbuf[N + c] = tv_word_a<LOGN>(tv, e);   // encrypted table: the a half from the row's a polynomial
            else accbuf[N + c] = 0u;
        }
    }
    wave_lds_sync();

    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
#pragma unroll 1
    for (int i = 0; i < a.steps; i++) {
        const int r = __builtin_amdgcn_readfirstlane((int)abar[i]);
        cmux_step<LOGN, L, BGBIT, true, DUAL, decltype(tvs)::ROUNDED>(accbuf, r, a.bk + (size_t)i * trgsw_cplx, twf, twi, twi_big, xbuf, lane);
    }

    if (a.mode == MODE_BLIND_ROTATE) {
        uint32_t* o = a.out + (size_t)g * 2 * N;
        for (int c = lane; c < 2 * N; c += 64) o[c] = accbuf[c];
        return;
    }

    // sample extract index 0 (trlwe.rs:110-121): a'_0 = a_0, a'_k = -a_{N-k}; b' = b_0
    uint32_t av[2 * R];
#pragma unroll
    for (int mm = 0; mm < 2 * R; mm++) av[mm] = accbuf[N + lane + 64 * mm];
    const uint32_t bprime = accbuf[0];
    wave_lds_sync();
#pragma unroll
    for (int mm = 0; mm < 2 * R; mm++) {
        const int c = lane + 64 * mm;
        accbuf[N + ((N - c) & (N - 1))] = (c == 0) ? av[mm] : (0u - av[mm]);
    }
    wave_lds_sync();
    if constexpr (decltype(tvs)::MANY) {      // many-LUT PBS (MODE_EXTRACT only): every output to the batch key switch's operand
        many_extract<N>(a.ext, a.ext_first + g, tv_shift(tvs), accbuf, lane, N, 64, lane);
        return;
    }
    key_switch_wave<LOGN, KS_T, KS_BB, KSQ>(accbuf + N, bprime, a.ksk, a.ksw, n, io.out, lane);
