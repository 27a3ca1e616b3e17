// rtfhe_kernels_trgsw_mac.hpp -- TRLWE x TRGSW multiply-accumulate: a sum of external products (include/rtfhe.h: rtfhe_trlwe_mul_trgsw_batch).
//
// One launch, a wave owns one sample and adds its K <= 8 terms in the frequency domain:
//   out[g] = (accumulate ? out[g] : 0) + fft( sum_k cross-spectra(S[s_idx[g][k]], x[x_idx[g][k]]) )      (TRGSWRepF::cross, trgsw.rs:264-306, with the
//                                                                                                         fold-add carried over the K terms)
// so that K products cost 6 K forward transforms, ONE pair of inverse transforms and one truncation.  The blocks are cmux_step's (rtfhe_kernels.hpp):
// the same digits, the same forward transform in its two halves with the selector's rows requested in between, the same unfused rr - ii, ir + ri
// fold-add in the same order (h = b, a; j = 0 .. l-1), the same inverse.  Its forward half (mac_forward) includes the loop over the digit rows
// that cmux_step includes, rtfhe_body_digit_rows.hpp: one text, and every kernel compiles to what it did when each file carried a copy.
// ROUNDED is cmux_step's.  Instantiated in rtfhe_trgsw_mac.hip.
//
// The sum reaches K * 2l * N * (Bg/2) * 2^31 = 2^51.6 (N = 1024) and 2^52.6 (N = 2048) at K = 8: above the 2^51 trunc_to_torus is exact below,
// inside the 2^53 of an exact double, so the conversion is trunc_to_torus_wide.
//
// A sample with an index outside the selector set or the rows is skipped whole and its output row stays as it was.
#pragma once

#include "rtfhe_kernels_cmux_tree.hpp"

namespace rtfhe {

constexpr int TRGSW_MAC_K_MAX = 8;

struct TrgswMacArgs {
    const cplx* tw;
    const cplx* sel;           // selector spectra, device layout [n_sel][2l][2][R][64]
    const int32_t* s_idx;      // [count][K], entry k = the selector of term k; null: sample g uses g * K + k
    const uint32_t* x;         // [n_x][2][N] (b then a); overlaps no part of `out`
    const int32_t* x_idx;      // [count][K], entry k = the row of term k; null: sample g uses g * K + k
    uint32_t* out;             // [count][2][N]
    int32_t* fault;            // set to 1 when a sample was skipped for an out-of-range index
    int32_t count, K;
    int32_t n_sel, n_x;
    int32_t accumulate;        // add into out instead of overwriting it
};

__device__ __forceinline__ int trgsw_mac_index(const int32_t* idx, long long g, int K, int k) { return idx ? idx[(size_t)g * K + k] : (int)(g * K + k); }

// are all 2 K indices of sample g in range?  (wave-uniform)
__device__ __forceinline__ bool trgsw_mac_ok(const TrgswMacArgs& a, long long g) {
    bool ok = true;
    for (int k = 0; k < a.K; k++) {
        ok = ok && (unsigned)trgsw_mac_index(a.s_idx, g, a.K, k) < (unsigned)a.n_sel;
        ok = ok && (unsigned)trgsw_mac_index(a.x_idx, g, a.K, k) < (unsigned)a.n_x;
    }
    return ok;
}

// The forward half of cmux_step<.., CMUX = false> on the row in rowbuf (LDS u32 [2][N], b then a), with the four running spectra kept by the
// caller: s_c <- s_c + hadamard(S.row(c, h, j), ifft_i32(digit_j(poly_h))) for h = b, a and j = 0 .. L-1, in that order.
template <int LOGN, int L, int BGBIT, bool DUAL, bool ROUNDED>
__device__ __forceinline__ void mac_forward(const uint32_t* __restrict__ rowbuf, const cplx* __restrict__ S, const cplx* __restrict__ twf,
                                            double* __restrict__ xbuf, int lane, double (&s0re)[Geo<LOGN>::R], double (&s0im)[Geo<LOGN>::R],
                                            double (&s1re)[Geo<LOGN>::R], double (&s1im)[Geo<LOGN>::R]) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    constexpr uint32_t MA = decomp_add(L, BGBIT, ROUNDED), MX = decomp_xor(L, BGBIT, ROUNDED);
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const uint32_t* poly = rowbuf + h * N;
        uint32_t u[2 * R];
#pragma unroll
        for (int mm = 0; mm < 2 * R; mm++) u[mm] = (poly[lane + 64 * mm] + MA) ^ MX;
#define RTFHE_DIGIT_ROW(jj) (S + (size_t)((h * L + jj) * 2) * R * 64 + lane)
#include "rtfhe_body_digit_rows.hpp"
    }
}

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_trlwe_mul_trgsw(const TrgswMacArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    static_assert(cmux_tree_lds_bytes<LOGN, WAVES>() <= (size_t)160 * 1024, "k_trlwe_mul_trgsw: the LDS carve of this (N, waves) shape passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = leveled_stage_twiddles<LOGN, WAVES>(smem, a.tw, tid);

    const long long g = (long long)blockIdx.x * WAVES + wave;
    if (g >= a.count) return;

    // every index of the sample is checked before anything of it is touched (a handful of wave-uniform loads): a bad sample is skipped whole
    if (!trgsw_mac_ok(a, g)) {
        if (a.fault) *a.fault = 1;
        return;
    }

    const WaveLds w = leveled_wave_lds<LOGN, WAVES>(smem, wave);
    double* xbuf = w.xbuf;
    uint32_t* rowbuf = w.accbuf;

    double s0re[R], s0im[R], s1re[R], s1im[R];
#pragma unroll
    for (int m = 0; m < R; m++) { s0re[m] = 0.0; s0im[m] = 0.0; s1re[m] = 0.0; s1im[m] = 0.0; }

    // N = 1024: the next term's row is requested under this term's transforms (a wave is alone on its SIMD: nothing else hides the miss of a
    // row read for the first time) and waits in 2N / 64 = 32 registers; at N = 2048 its 64 registers would go to scratch, the row is read in place
    constexpr bool PREFETCH = LOGN == 10;
    constexpr int W = 2 * N / 64;
    uint32_t nxt[PREFETCH ? W : 1];
    if constexpr (PREFETCH) {
        const uint32_t* row = a.x + (size_t)__builtin_amdgcn_readfirstlane(trgsw_mac_index(a.x_idx, g, a.K, 0)) * 2 * N;
#pragma unroll
        for (int i = 0; i < W; i++) nxt[i] = row[lane + 64 * i];
    }

    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
#pragma unroll 1
    for (int k = 0; k < a.K; k++) {
        const int sk = __builtin_amdgcn_readfirstlane(trgsw_mac_index(a.s_idx, g, a.K, k));
        wave_lds_sync();      // the previous term's digits have been read
        if constexpr (PREFETCH) {
#pragma unroll
            for (int i = 0; i < W; i++) rowbuf[lane + 64 * i] = nxt[i];
            wave_lds_sync();
            if (k + 1 < a.K) {
                const uint32_t* row = a.x + (size_t)__builtin_amdgcn_readfirstlane(trgsw_mac_index(a.x_idx, g, a.K, k + 1)) * 2 * N;
#pragma unroll
                for (int i = 0; i < W; i++) nxt[i] = row[lane + 64 * i];
            }
            __builtin_amdgcn_sched_barrier(0);
        } else {
            const uint32_t* row = a.x + (size_t)__builtin_amdgcn_readfirstlane(trgsw_mac_index(a.x_idx, g, a.K, k)) * 2 * N;
            for (int c = lane; c < 2 * N; c += 64) rowbuf[c] = row[c];
            wave_lds_sync();
        }
        mac_forward<LOGN, L, BGBIT, DUAL, ROUNDED>(rowbuf, a.sel + (size_t)sk * trgsw_cplx, TwStage<LOGN>::fwd(tw), xbuf, lane, s0re, s0im, s1re, s1im);
    }

    // the 2/N input scaling of the reference (fft_processor_spqlios.cpp:158) is folded into the untwist twiddles
    uint32_t* o = a.out + (size_t)g * 2 * N;
    const bool acc = a.accumulate != 0;
#pragma unroll 1
    for (int comp = 0; comp < 2; comp++) {
        uint32_t* poly = o + comp * N;
        // the old polynomial is requested before the inverse transform and consumed after it: the transform covers its latency
        uint32_t old0[R], old1[R];
#pragma unroll
        for (int m = 0; m < R; m++) { old0[m] = 0u; old1[m] = 0u; }
        if (acc) {
#pragma unroll
            for (int m = 0; m < R; m++) { old0[m] = poly[lane + 64 * m]; old1[m] = poly[lane + 64 * m + P]; }
        }
        __builtin_amdgcn_sched_barrier(0);
        double re[R], im[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            re[m] = comp ? s1re[m] : s0re[m];
            im[m] = comp ? s1im[m] : s0im[m];
        }
        fft_inverse<LOGN, DUAL>(re, im, TwStage<LOGN>::inv_small(tw), TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);
#pragma unroll
        for (int m = 0; m < R; m++) {
            poly[lane + 64 * m] = old0[m] + trunc_to_torus_wide(re[m]);
            poly[lane + 64 * m + P] = old1[m] + trunc_to_torus_wide(im[m]);
        }
    }
}

}  // namespace rtfhe
