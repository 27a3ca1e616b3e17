// rtfhe_kernels_trlwe_auto.hpp -- TRLWE key switching: automorphisms X -> X^t and re-keying (include/rtfhe.h: rtfhe_trlwe_auto_batch).
//
// One launch, a wave owns one row and runs all steps of the call's program on the wave-private row in LDS.  A step with entry e of the
// switching key K and exponent t = t[e], on the row x = (b, a):
//   a' = sigma_t(a), b' = sigma_t(b)                                   sigma_t(p)[j t mod 2N mod N] = +-p[j], negated when j t mod 2N >= N
//   sum_c = sum_j hadamard(K[e].row(c, j), ifft_i32(digit_j(a')))      c = 0 (b), 1 (a);  j = 0 .. l-1 in order, fold-add from 0.0
//   y = (b' + fft_u32(sum_0), fft_u32(sum_1));   x <- y  or  x <- x + y
// i.e. (sigma_t b, 0) + cross(T, (sigma_t a, 0)) with T the TRGSW whose rows (c, h = b, j) are K[e]'s and whose rows (c, h = a, j) are zero
// (TRGSWRepF::cross, trgsw.rs:264-306).  The blocks are cmux_step's (rtfhe_kernels.hpp): the same digits, the same forward transform in its two
// halves with the key's two rows of the digit requested in between, the same unfused rr - ii, ir + ri fold-add, the same inverse and the same
// truncation -- a single product stays below l * N * (Bg/2) * 2^31 < 2^49, so the narrow trunc_to_torus is exact.  The forward half is
// the loop over the digit rows that cmux_step and mac_forward include (rtfhe_body_digit_rows.hpp), for ONE polynomial, the rows read from
// K[e]: one text, and every kernel compiles to what it did when each file carried a copy.  ROUNDED is cmux_step's.  Instantiated in
// rtfhe_trlwe_auto.hip.
//
// The program (entries, add flags) is the host's and was checked there (rtfhe_trlwe_auto_plan): the kernel has no index to refuse.
#pragma once

#include "rtfhe_kernels_cmux_tree.hpp"

namespace rtfhe {

constexpr int TRLWE_AUTO_MAX_STEPS = 16;

struct TrlweAutoArgs {
    const cplx* tw;
    const cplx* key;           // switching-key spectra, device layout [n_t][l][2][R][64]: row j of entry e as (b, a)
    const uint32_t* in;        // [count][2][N] (b then a); may be exactly `out`
    uint32_t* out;             // [count][2][N]
    int32_t count, n_steps;
    uint32_t add;              // bit k: step k adds into the row instead of replacing it
    int32_t entry[TRLWE_AUTO_MAX_STEPS];      // the key entry of step k, copied from the caller's host array when the launch is enqueued
    int32_t tinv[TRLWE_AUTO_MAX_STEPS];       // t[entry[k]]^-1 mod 2N (rtfhe_trlwe_auto_inverse)
};

// sigma_t(p)[c] by the inverse map: with q = c t^-1 mod 2N, +p[q] for q < N and -p[q - N] above.  Consecutive lanes advance the LDS dword
// index by the odd t^-1: the 32 lanes of a ds_read_b32 group fall on 32 different banks.
template <int LOGN>
__device__ __forceinline__ uint32_t auto_coef(const uint32_t* __restrict__ p, int c, int tinv) {
    constexpr int N = 1 << LOGN;
    const int q = (c * tinv) & (2 * N - 1);
    const uint32_t v = p[q & (N - 1)];
    return (q >> LOGN) ? (0u - v) : v;
}

// One step on the wave-private row in rowbuf (LDS u32 [2][N], b then a).  K: the entry's spectra [l][2][R][64].
// The a half is written back first, behind its own inverse transform: every lane gathered a' at the top of the step, and the gather of b' still
// reads the b half, which is written last -- behind a wave_lds_sync, so that no lane stores a word of b another lane has yet to gather.
template <int LOGN, int L, int BGBIT, bool DUAL, bool ROUNDED>
__device__ __forceinline__ void auto_step(uint32_t* __restrict__ rowbuf, int tinv, bool add, const cplx* __restrict__ K, const cplx* __restrict__ twf,
                                          const cplx* __restrict__ twi, const cplx* __restrict__ twi_big, double* __restrict__ xbuf, int lane) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R;
    constexpr uint32_t MA = decomp_add(L, BGBIT, ROUNDED), MX = decomp_xor(L, BGBIT, ROUNDED);

    double s0re[R], s0im[R], s1re[R], s1im[R];
#pragma unroll
    for (int m = 0; m < R; m++) { s0re[m] = 0.0; s0im[m] = 0.0; s1re[m] = 0.0; s1im[m] = 0.0; }

    {
        uint32_t u[2 * R];
#pragma unroll
        for (int mm = 0; mm < 2 * R; mm++) u[mm] = (auto_coef<LOGN>(rowbuf + N, lane + 64 * mm, tinv) + MA) ^ MX;
#define RTFHE_DIGIT_ROW(jj) (K + (size_t)(jj * 2) * R * 64 + lane)
#include "rtfhe_body_digit_rows.hpp"
    }

    // the 2/N input scaling of the reference (fft_processor_spqlios.cpp:158) is folded into the untwist twiddles
#pragma unroll 1
    for (int comp = 1; comp >= 0; comp--) {
        double re[R], im[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            re[m] = comp ? s1re[m] : s0re[m];
            im[m] = comp ? s1im[m] : s0im[m];
        }
        fft_inverse<LOGN, DUAL>(re, im, twi, twi_big, xbuf, lane);
        uint32_t* poly = rowbuf + comp * N;
        uint32_t y0[R], y1[R];
#pragma unroll
        for (int m = 0; m < R; m++) { y0[m] = trunc_to_torus(re[m]); y1[m] = trunc_to_torus(im[m]); }
        if (comp == 0) {
#pragma unroll
            for (int m = 0; m < R; m++) {
                y0[m] += auto_coef<LOGN>(rowbuf, lane + 64 * m, tinv);
                y1[m] += auto_coef<LOGN>(rowbuf, lane + 64 * m + P, tinv);
            }
        }
        if (add) {
#pragma unroll
            for (int m = 0; m < R; m++) { y0[m] += poly[lane + 64 * m]; y1[m] += poly[lane + 64 * m + P]; }
        }
        wave_lds_sync();
#pragma unroll
        for (int m = 0; m < R; m++) { poly[lane + 64 * m] = y0[m]; poly[lane + 64 * m + P] = y1[m]; }
    }
    wave_lds_sync();
}

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_trlwe_auto(const TrlweAutoArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    static_assert(cmux_tree_lds_bytes<LOGN, WAVES>() <= (size_t)160 * 1024, "k_trlwe_auto: the LDS carve of this (N, waves) shape passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = leveled_stage_twiddles<LOGN, WAVES>(smem, a.tw, tid);

    const long long g = (long long)blockIdx.x * WAVES + wave;
    if (g >= a.count) return;

    const WaveLds w = leveled_wave_lds<LOGN, WAVES>(smem, wave);
    double* xbuf = w.xbuf;
    uint32_t* rowbuf = w.accbuf;

    // the whole row goes into LDS before anything is stored: out may be the input buffer
    const uint32_t* row = a.in + (size_t)g * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) rowbuf[c] = row[c];
    wave_lds_sync();

    const size_t entry_cplx = (size_t)L * 2 * R * 64;
#pragma unroll 1
    for (int k = 0; k < a.n_steps; k++)
        auto_step<LOGN, L, BGBIT, DUAL, ROUNDED>(rowbuf, a.tinv[k], (a.add >> k) & 1u, a.key + (size_t)a.entry[k] * entry_cplx, TwStage<LOGN>::fwd(tw),
                                                 TwStage<LOGN>::inv_small(tw), TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);

    // 64 lanes x 4 bytes: every store instruction of the wave is one whole 256-byte run
    uint32_t* o = a.out + (size_t)g * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) o[c] = rowbuf[c];
}

}  // namespace rtfhe
