// rtfhe_kernels_pbs_mb_wg.hpp -- the latency shape of the multi-bit blind rotation (rtfhe_kernels_pbs_mb.hpp): N = 1024, one gate per workgroup
// of six waves.  Wave r owns digit row (h, jj) = (r / 3, r % 3) of every step: it decomposes polynomial h of the accumulator, transforms digit
// jj forward, combines its own two key rows over the group's subsets (rtfhe_body_mb_combine.hpp, the text mb_step's fold includes) and
// multiplies -- one sixth of mb_step's forward work, side by side.
//
// The six products meet in cmux_step's fold order, so that every word equals k_pbs_mb's: one running sum per component and point in LDS, to
// which wave 0 stores 0.0 + its product and waves 1 .. 5 add theirs in turn, a barrier between turns (row r of mb_step's loop is turn r).  Waves
// 0 and 1 then transform component 0 and 1 back and add the truncated words into the accumulator.  The running sum takes 16 KiB where six
// partial spectra would take 96 KiB -- with the 32 KiB of twiddles those would pass the 160 KiB of a CU.
// The point is the halved chain of dependent steps, not a tuned schedule: barriers are workgroup-wide, four waves idle during the inverse.
#pragma once

#include "rtfhe_kernels_pbs_mb.hpp"

namespace rtfhe {

constexpr int MB_WG_WAVES = 2 * MB_L;      // one wave per digit row

// tw | the roots table W[2N] | six exchange buffers | running sum [2][R][64] cplx | accumulator [2][N] | abar [npad]
__host__ __device__ constexpr size_t pbs_mb_wg_lds_bytes(int npad) {
    return (size_t)TwStage<10>::LDS_CPLX * sizeof(cplx) + (size_t)2 * Geo<10>::N * sizeof(cplx) + (size_t)MB_WG_WAVES * Geo<10>::XSLOTS * sizeof(double) +
           (size_t)2 * Geo<10>::P * sizeof(cplx) + (size_t)2 * Geo<10>::N * 4 + (size_t)npad * 4;
}

template <bool ROUNDED>
__global__ __launch_bounds__(64 * MB_WG_WAVES, 1) void k_pbs_mb_wg(const PbsMbArgs a) {
    constexpr int LOGN = 10, L = MB_L, BGBIT = MB_BGBIT, WAVES = MB_WG_WAVES, THREADS = 64 * WAVES;
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R, MASK = 2 * N - 1;
    constexpr uint32_t MA = decomp_add(L, BGBIT, ROUNDED), MX = decomp_xor(L, BGBIT, ROUNDED);
    constexpr size_t TRGSW = (size_t)2 * L * 2 * R * 64;
    static_assert(pbs_mb_wg_lds_bytes(256 * MB_KSQ) <= (size_t)160 * 1024, "k_pbs_mb_wg: the LDS carve passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = reinterpret_cast<cplx*>(smem);
    TwStage<LOGN>::stage(tw, a.tw, tid, THREADS);
    cplx* roots = tw + TwStage<LOGN>::LDS_CPLX;      // W in LDS (rtfhe_kernels_pbs_mb.hpp: mb_roots_in_lds)
    for (int idx = tid; idx < 2 * N; idx += THREADS) roots[idx] = a.roots[idx];
    __syncthreads();

    const int g = blockIdx.x;      // < count: the grid is count workgroups
    const TvLut tvs{a.tv, a.tv_idx, a.n_tv, a.fault};
    const auto tv = tv_row(tvs, g, N);
    if (!tv.ok()) {                // skipped, by all six waves alike: the output row keeps its words, *fault is set
        park_row<N>(a, a.out, g, tid, THREADS);
        return;
    }

    unsigned char* base = smem + ((size_t)TwStage<LOGN>::LDS_CPLX + 2 * N) * sizeof(cplx);
    double* xbuf = reinterpret_cast<double*>(base) + (size_t)wave * G::XSLOTS;
    cplx* sum = reinterpret_cast<cplx*>(base + (size_t)WAVES * G::XSLOTS * sizeof(double)) + lane;      // [comp][m][64]
    uint32_t* accbuf = reinterpret_cast<uint32_t*>(base + (size_t)WAVES * G::XSLOTS * sizeof(double) + (size_t)2 * P * sizeof(cplx));
    uint32_t* abar = accbuf + 2 * N;
    const cplx* twf = TwStage<LOGN>::fwd(tw);
    const cplx* twi = TwStage<LOGN>::inv_small(tw);
    const cplx* twi_big = TwStage<LOGN>::inv_big(tw, a.tw);

    const int n = a.n;
    const uint32_t* in = a.in + (size_t)g * ((size_t)n + 1);
    const GateIo io{in, in, a.out + (size_t)g * ((size_t)n + 1), OP_COPY, true};
    gate_mask<LOGN>(io, tvs, n, abar, tid, THREADS);
    __syncthreads();
    {
        const int bbar = (int)abar[n];
        for (int c = tid; c < 2 * N; c += THREADS) accbuf[c] = acc_start<LOGN>(tvs, tv, bbar, c);
    }
    __syncthreads();

    int q[R];
#pragma unroll
    for (int m = 0; m < R; m++) q[m] = a.qmap[m * 64 + lane];

    const int h = wave / L, jj = wave - h * L;
    const int gb = a.g, full = n / gb, groups = (n + gb - 1) / gb, jfull = (1 << gb) - 1;
#pragma unroll 1
    for (int t = 0; t < groups; t++) {
        const int bits = t < full ? gb : n - full * gb, i0 = t * gb, J = (1 << bits) - 1;
        const int r0 = __builtin_amdgcn_readfirstlane((int)abar[i0]);
        const int r1 = bits > 1 ? __builtin_amdgcn_readfirstlane((int)abar[i0 + 1]) : 0;
        const int r2 = bits > 2 ? __builtin_amdgcn_readfirstlane((int)abar[i0 + 2]) : 0;
        const cplx* row = a.mbk + (size_t)t * jfull * TRGSW + (size_t)((h * L + jj) * 2) * R * 64 + lane;

        // this wave's digit row: mb_step's loop body at (h, jj), the products kept instead of folded
        double re[R], im[R];
        {
            const uint32_t* poly = accbuf + h * N;
#pragma unroll
            for (int m = 0; m < R; m++) {
                re[m] = (double)decomp_digit((poly[lane + 64 * m] + MA) ^ MX, BGBIT, jj);
                im[m] = (double)decomp_digit((poly[lane + 64 * (R + m)] + MA) ^ MX, BGBIT, jj);
            }
        }
        fft_forward_a<LOGN, false>(re, im, twf, xbuf, lane);
        __builtin_amdgcn_sched_barrier(0);
        cplx b0[R], b1[R];
#pragma unroll
        for (int m = 0; m < R; m++) { b0[m] = row[m * 64]; b1[m] = row[(R + m) * 64]; }
        __builtin_amdgcn_sched_barrier(0);
        fft_forward_b<LOGN, false>(re, im, twf, xbuf, lane);
        cplx p0[R], p1[R];
        auto product = [&](cplx (&p)[R], const cplx (&b)[R], int comp) {
            cplx K[R];
#include "rtfhe_body_mb_combine.hpp"
#pragma unroll
            for (int m = 0; m < R; m++) {
                const double ii = K[m].y * im[m], rr = K[m].x * re[m], ri = K[m].x * im[m], ir = K[m].y * re[m];
                p[m].x = rr - ii;
                p[m].y = ir + ri;
            }
        };
        product(p0, b0, 0);
        product(p1, b1, 1);

        // the fold, row by row in mb_step's order: turn k is wave k's
#pragma unroll 1
        for (int k = 0; k < WAVES; k++) {
            if (wave == k) {
#pragma unroll
                for (int m = 0; m < R; m++) {
                    cplx s0 = make_double2(0.0, 0.0), s1 = make_double2(0.0, 0.0);
                    if (k) { s0 = sum[m * 64]; s1 = sum[(R + m) * 64]; }
                    s0.x = s0.x + p0[m].x; s0.y = s0.y + p0[m].y;
                    s1.x = s1.x + p1[m].x; s1.y = s1.y + p1[m].y;
                    sum[m * 64] = s0; sum[(R + m) * 64] = s1;
                }
            }
            __syncthreads();
        }

        // waves 0 and 1: component `wave` back, truncated and added into the accumulator (mb_step's tail)
        if (wave < 2) {
#pragma unroll
            for (int m = 0; m < R; m++) { const cplx s = sum[(wave * R + m) * 64]; re[m] = s.x; im[m] = s.y; }
            fft_inverse<LOGN, false>(re, im, twi, twi_big, xbuf, lane);
            uint32_t* poly = accbuf + wave * N;
#pragma unroll
            for (int m = 0; m < R; m++) {
                const int c = lane + 64 * m;
                poly[c] += trunc_to_torus(re[m]);
                poly[c + P] += trunc_to_torus(im[m]);
            }
        }
        __syncthreads();
    }

    // sample extract index 0 of the a-polynomial in place (extract_flip's step, four words each of the first 256 threads; every wave meets the barriers)
    {
        uint32_t* apoly = accbuf + N;
        uint32_t av[4];
        if (tid < 256)
#pragma unroll
            for (int k = 0; k < 4; k++) av[k] = apoly[tid + 256 * k];
        __syncthreads();
        if (tid < 256)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int c = tid + 256 * k;
                apoly[(N - c) & (N - 1)] = (c == 0) ? av[k] : (0u - av[k]);
            }
        __syncthreads();
    }
    if (a.ext) {
        gate_extract_store<N>(a.ext, io.out, tvs, n, g, accbuf, accbuf + N, tid, N, THREADS, tid, tid, THREADS);
        return;
    }
    if (wave == 0) key_switch_wave<LOGN, MB_KS_T, MB_KS_BB, MB_KSQ>(accbuf + N, accbuf[0], a.ksk, a.ksw, n, io.out, lane);
}

}  // namespace rtfhe
