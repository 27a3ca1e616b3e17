// rtfhe_kernels_pbs_mb.hpp -- multi-bit blind rotation (include/rtfhe.h: rtfhe_pbs_mb_batch): a programmable bootstrap whose blind rotation
// takes g = 2 or 3 key bits per step, ceil(n / g) dependent steps instead of n.  One step per group t of key bits [t g, min(n, t g + g)):
//
//   acc <- acc + (Sum_j F_{e_j} . BK_{t,j}) [.] acc,    j = 1 .. J = 2^g' - 1 over the non-empty subsets of the group's g' bits,
//
// BK_{t,j} the TRGSW sample of "exactly the bits of j are set" (rtfhe_keygen.cpp: mbk_material), e_j = Sum_{q in j} abar_{t g + q} mod 2N the
// rotation the single-bit PBS would have made for those bits, and F_e the spectrum of X^e - 1 in the transform's own point order:
// F_e[p] = W[(e q_p) mod 2N] - 1 with W[t] = exp(i pi t / N) and q_p the odd exponent of point p (both tables: rtfhe_mb_plan.cpp, uploaded as
// data).  Exactly one subset -- or none -- holds 1, so the bracket encrypts X^e - 1 for the e of the bits that are set, and the step is the
// product of the group's single-bit CMUX steps.
//
// mb_step is cmux_step<.., CMUX = false> (rtfhe_kernels.hpp) with the key combination where that one reads its row pair: the same
// decomposition of acc itself, the same transforms, the same fold order, inverse and truncation, the truncated product ADDED into acc.  Its
// digit loop MIRRORS rtfhe_body_digit_rows.hpp -- the loop cmux_step includes -- and keeps its own text because its fold differs; a change there
// is made here too.  The key combination is rtfhe_body_mb_combine.hpp, one text for this file's fold and k_pbs_mb_wg's product.  The tail
// (inverse, truncation, += into acc) is cmux_step<.., CMUX = true>'s, kept as its own text: worded as cmux_step's it changes k_pbs_mb<11>,
// worded as this one it changes the N = 2048 kernels built on cmux_step (profiles/r37/README.md).  Every
// product and sum is rounded on its own (the library is built without contraction), in this order per digit row, component and point:
//   K = F_{e_1} B_1;  K = K + F_{e_j} B_j for j = 2 .. J;  each complex product (rr - ii, ir + ri) as in cmux_step's hadamard;
// then K stands where cmux_step has b0 / b1.  No subset is skipped when e_j = 0 (F_0 = 0 exactly: W[0] = 1).
// J and the e_j are wave-uniform and live in scalar registers; W is read by a computed index.  The row pair of subset 1 is requested where
// cmux_step requests its pair, behind fft_forward_a; the others one component at a time as they are combined: at g = 3 seven pairs cannot be live.
//
// A skipped gate (table index out of range) in the extract form parks its output row for k_rows_restore: the one parked-row rule of
// rtfhe_kernels.hpp (park_row), with (tv_idx, 1, n_tv) as the restore's index rule.  In the fused form nothing is stored and the row keeps its words.
//
// k_pbs_mb: a wave per gate in k_trgsw_rotate's launch shape (four waves per workgroup, the accumulator in LDS across all steps), N = 1024
// and 2048, any count, the frame of rtfhe_gate_frame.hpp around the step loop.  Instantiated in rtfhe_pbs_mb.hip.
#pragma once

#include "rtfhe_kernels.hpp"

namespace rtfhe {

constexpr int MB_WAVES = 4;
constexpr int MB_L = 3, MB_BGBIT = 6, MB_KS_T = 8, MB_KS_BB = 2, MB_KSQ = 3;      // the one parameter set every bootstrap kernel is instantiated for

struct PbsMbArgs {
    const cplx* tw;
    const cplx* mbk;           // key spectra, [n_trgsw][2l][2][R][64]: groups in order, subsets j = 1 .. J ascending
    const cplx* roots;         // W[2N]
    const int32_t* qmap;       // [N/2]: q_p of spectrum point p = m * 64 + lane
    const uint32_t* ksk;       // the fused form's key-switching key (ks_accumulate's layout)
    const uint32_t* in;        // [count][n+1]
    uint32_t* out;             // [count][n+1]
    uint32_t* ext;             // extract form: lvl1 samples in the batch key switch's operand order; null: the kernel switches keys itself
    const uint32_t* tv;        // [n_tv][N] test polynomials
    const int32_t* tv_idx;     // [count] or null (table 0)
    int32_t* fault;            // set to 1 when a gate was skipped for a table index out of range
    int32_t n_tv, count, n, g, ksw, npad;
};

// e_j of subset j from the group's rotations (wave-uniform)
__device__ __forceinline__ int mb_exponent(int j, int r0, int r1, int r2, int mask) {
    return (((j & 1) ? r0 : 0) + ((j & 2) ? r1 : 0) + ((j & 4) ? r2 : 0)) & mask;
}

// One multi-bit step on the wave-private accumulator in LDS.  group: the group's first TRGSW; J its subsets; r0 .. r2 its rotations (0 past
// the group's bits); q: this lane's R point exponents.
template <int LOGN, int L, int BGBIT, bool DUAL, bool ROUNDED>
__device__ __forceinline__ void mb_step(uint32_t* __restrict__ accbuf, int J, int r0, int r1, int r2, const cplx* __restrict__ group,
                                        const cplx* __restrict__ roots, const int (&q)[Geo<LOGN>::R], const cplx* __restrict__ twf,
                                        const cplx* __restrict__ twi, const cplx* __restrict__ twi_big, double* __restrict__ xbuf, int lane) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R, MASK = 2 * N - 1;
    constexpr uint32_t MA = decomp_add(L, BGBIT, ROUNDED), MX = decomp_xor(L, BGBIT, ROUNDED);
    constexpr size_t TRGSW = (size_t)2 * L * 2 * R * 64;

    double s0re[R], s0im[R], s1re[R], s1im[R];
#pragma unroll
    for (int m = 0; m < R; m++) { s0re[m] = 0.0; s0im[m] = 0.0; s1re[m] = 0.0; s1im[m] = 0.0; }

#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const uint32_t* poly = accbuf + h * N;
        uint32_t u[2 * R];
#pragma unroll
        for (int mm = 0; mm < 2 * R; mm++) u[mm] = (poly[lane + 64 * mm] + MA) ^ MX;
        // rtfhe_body_digit_rows.hpp mirrored: the same loop with the key combination in the fold
#pragma unroll 1
        for (int jj = 0; jj < L; jj++) {
            const cplx* row = group + (size_t)((h * L + jj) * 2) * R * 64 + lane;
            double re[R], im[R];
#pragma unroll
            for (int m = 0; m < R; m++) {
                re[m] = (double)decomp_digit(u[m], BGBIT, jj);
                im[m] = (double)decomp_digit(u[R + m], BGBIT, jj);
            }
            fft_forward_a<LOGN, DUAL>(re, im, twf, xbuf, lane);
            // subset 1's row pair is requested here, as cmux_step requests its pair
            __builtin_amdgcn_sched_barrier(0);
            cplx b0[R], b1[R];
#pragma unroll
            for (int m = 0; m < R; m++) { b0[m] = row[m * 64]; b1[m] = row[(R + m) * 64]; }
            __builtin_amdgcn_sched_barrier(0);
            fft_forward_b<LOGN, DUAL>(re, im, twf, xbuf, lane);
            // the key combination of one component, then its hadamard + fold-add (cmux_step's, K for b)
            auto fold = [&](double (&sre)[R], double (&sim)[R], const cplx (&b)[R], int comp) {
                cplx K[R];
#include "rtfhe_body_mb_combine.hpp"
#pragma unroll
                for (int m = 0; m < R; m++) {
                    const double ii = K[m].y * im[m], rr = K[m].x * re[m], ri = K[m].x * im[m], ir = K[m].y * re[m];
                    sre[m] = sre[m] + (rr - ii);
                    sim[m] = sim[m] + (ir + ri);
                }
            };
            fold(s0re, s0im, b0, 0);
            fold(s1re, s1im, b1, 1);
        }
    }

#pragma unroll 1
    for (int comp = 0; comp < 2; comp++) {
        double re[R], im[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            re[m] = comp ? s1re[m] : s0re[m];
            im[m] = comp ? s1im[m] : s0im[m];
        }
        fft_inverse<LOGN, DUAL>(re, im, twi, twi_big, xbuf, lane);
        uint32_t* poly = accbuf + comp * N;
#pragma unroll
        for (int m = 0; m < R; m++) {
            const int c = lane + 64 * m;
            poly[c] += trunc_to_torus(re[m]);
            poly[c + P] += trunc_to_torus(im[m]);
        }
    }
    wave_lds_sync();
}

// At N = 1024 the roots table (32 KiB) is staged into LDS behind the waves' carves: the key combination gathers 16 bytes per lane at an index that
// differs in every lane, two gathers per point and subset, and from global memory those gathers were most of a step (profiles/r34).  At
// N = 2048 the table (64 KiB) does not fit beside four waves and stays in global memory.
__host__ __device__ constexpr bool mb_roots_in_lds(int logn) { return logn == 10; }
template <int LOGN>
__host__ __device__ constexpr size_t pbs_mb_lds_bytes(int npad) {
    return bootstrap_lds_bytes<LOGN>(MB_WAVES, npad, bootstrap_dual_xbuf(LOGN, MB_WAVES)) + (mb_roots_in_lds(LOGN) ? (size_t)2 * Geo<LOGN>::N * sizeof(cplx) : 0);
}

template <int LOGN, bool ROUNDED>
__global__ __launch_bounds__(64 * MB_WAVES, 1) void k_pbs_mb(const PbsMbArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R, WAVES = MB_WAVES;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = reinterpret_cast<cplx*>(smem);
    TwStage<LOGN>::stage(tw, a.tw, tid, 64 * WAVES);
    const cplx* roots = a.roots;
    if constexpr (mb_roots_in_lds(LOGN)) {
        cplx* wl = reinterpret_cast<cplx*>(smem + (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)WAVES * bootstrap_wave_lds_bytes<LOGN>(a.npad, DUAL));
        for (int idx = tid; idx < 2 * N; idx += 64 * WAVES) wl[idx] = a.roots[idx];
        roots = wl;
    }
    __syncthreads();
    // from here on waves never synchronise with each other

    const int g = blockIdx.x * WAVES + wave;
    if (g >= a.count) return;
    const TvLut tvs{a.tv, a.tv_idx, a.n_tv, a.fault};
    const auto tv = tv_row(tvs, g, N);
    if (!tv.ok()) {            // skipped: the output row keeps its words (extract form: parked for k_rows_restore, rtfhe_kernels.hpp), *fault is set
        park_row<N>(a, a.out, g, lane, 64);
        return;
    }

    unsigned char* wbase = smem + (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)wave * bootstrap_wave_lds_bytes<LOGN>(a.npad, DUAL);
    double* xbuf = reinterpret_cast<double*>(wbase);
    uint32_t* accbuf = reinterpret_cast<uint32_t*>(wbase + (size_t)G::XSLOTS * sizeof(double) * (DUAL ? 2 : 1));
    uint32_t* abar = accbuf + 2 * N;
    const cplx* twf = TwStage<LOGN>::fwd(tw);
    const cplx* twi = TwStage<LOGN>::inv_small(tw);
    const cplx* twi_big = TwStage<LOGN>::inv_big(tw, a.tw);

    const int n = a.n;
    const uint32_t* in = a.in + (size_t)g * ((size_t)n + 1);
    const GateIo io{in, in, a.out + (size_t)g * ((size_t)n + 1), OP_COPY, true};
    gate_mask<LOGN>(io, tvs, n, abar, lane, 64);
    wave_lds_sync();
    {
        const int bbar = (int)abar[n];
#pragma unroll
        for (int mm = 0; mm < 2 * R; mm++) {
            const int c = lane + 64 * mm;
            accbuf[c] = acc_start<LOGN>(tvs, tv, bbar, c);
            accbuf[N + c] = acc_start<LOGN>(tvs, tv, bbar, N + c);
        }
    }
    wave_lds_sync();

    int q[R];
#pragma unroll
    for (int m = 0; m < R; m++) q[m] = a.qmap[m * 64 + lane];

    const int gb = a.g, full = n / gb, groups = (n + gb - 1) / gb, jfull = (1 << gb) - 1;
    const size_t trgsw_cplx = (size_t)2 * MB_L * 2 * R * 64;
#pragma unroll 1
    for (int t = 0; t < groups; t++) {
        const int bits = t < full ? gb : n - full * gb, i0 = t * gb;
        const int r0 = __builtin_amdgcn_readfirstlane((int)abar[i0]);
        const int r1 = bits > 1 ? __builtin_amdgcn_readfirstlane((int)abar[i0 + 1]) : 0;
        const int r2 = bits > 2 ? __builtin_amdgcn_readfirstlane((int)abar[i0 + 2]) : 0;
        mb_step<LOGN, MB_L, MB_BGBIT, DUAL, ROUNDED>(accbuf, (1 << bits) - 1, r0, r1, r2, a.mbk + (size_t)t * jfull * trgsw_cplx, roots, q, twf, twi, twi_big,
                                                     xbuf, lane);
    }

    extract_flip<N, 2 * R>(accbuf + N, lane, 64, [] { wave_lds_sync(); });
    wave_lds_sync();
    if (a.ext) {
        gate_extract_store<N>(a.ext, io.out, tvs, n, g, accbuf, accbuf + N, lane, N, 64, lane, lane, 64);
        return;
    }
    key_switch_wave<LOGN, MB_KS_T, MB_KS_BB, MB_KSQ>(accbuf + N, accbuf[0], a.ksk, a.ksw, n, io.out, lane);
}

}  // namespace rtfhe
