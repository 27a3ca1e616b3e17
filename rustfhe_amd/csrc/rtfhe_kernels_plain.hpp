// rtfhe_kernels_plain.hpp -- the exact TRLWE x plain-polynomial product (include/rtfhe.h: rtfhe_plain_create, rtfhe_trlwe_mul_plain_batch[_dev]):
//   out[g] = (accumulate ? out[g] : 0) + sum_{k < K} w[w_idx[g][k]] * x[x_idx[g][k]]      in Z_{2^32}[X]/(X^N + 1), both polynomials of the row.
//
// The split-FFT exact backend's arithmetic (rtfhe_xfft.hpp) with the roles reversed: there the small operand (the digits) is transformed at run
// time and the 32-bit one (the key) is split once; here the small operand (the weights, total l1 norm K * wmax <= 192 N: the same
// rows * N * digit_max the backend is proven at) is transformed ONCE, by k_plain_build, and the 32-bit operand (the ciphertext) is split into signed
// 16-bit halves x = 2^16 hi + lo when it is read.  The two sums  sum_k w_k (*) hi_k  and  sum_k w_k (*) lo_k  stay below 192 N 2^15 = 2^32.6
// (N = 1024) / 2^33.6 (N = 2048), inside MAGIC's 2^35; each comes out of its own inverse transform, is rounded by the magic-number addition and
// the halves are recombined mod 2^32 in integer registers.  Exact: the result does not depend on the backend and adds no noise of its own.
//   N = 1024: one wave per (sample, polynomial), four waves per workgroup   (k_external_product_xfft's shape)
//   N = 2048: two waves per (sample, polynomial), wave h owning half h of every spectrum; the last inverse stage is traded through LDS behind
//             the workgroup's barrier                                       (k_external_product_xfft2's shape)
// Lane <-> coefficient is lane + 64 m: every wave load and store of a row is whole 256-byte runs.
#pragma once

#include "rtfhe_kernels_xfft2.hpp"

namespace rtfhe {

constexpr int PLAIN_K_MAX = 8;       // terms per product (rtfhe_plain_plan.h: RTFHE_PLAIN_K_MAX)
constexpr int PLAIN_WAVES = 4;       // N = 1024: waves per workgroup

// ---- weights -> spectra: k_xbk_build / k_xbk_build2 without the split ----
struct PlainBuildArgs {
    const cplx* xtw;
    const int32_t* w;         // [n_w][N]
    cplx* spec;               // N = 1024: [n_w][512]; N = 2048: [n_w][2 halves][512]
    int32_t count;            // n_w
};

template <int LOGN, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_plain_build(const PlainBuildArgs a) {
    typedef Geo<10> G;
    constexpr int N = 1 << LOGN, P = 512, R = 8, HALVES = LOGN == 11 ? 2 : 1;
    constexpr int TW_TOTAL = LOGN == 11 ? xfft::XTw2::TOTAL : xfft::XTw::TOTAL;
    static_assert(LOGN == 10 || LOGN == 11, "N = 1024 or 2048");
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int idx = tid; idx < TW_TOTAL; idx += 64 * WAVES) tw[idx] = a.xtw[idx];
    __syncthreads();
    double* xbuf = reinterpret_cast<double*>(smem + (size_t)TW_TOTAL * sizeof(cplx)) + (size_t)wave * 2 * G::XSLOTS;
    // work item = (polynomial, spectrum half)
    for (int item = blockIdx.x * WAVES + wave; item < HALVES * a.count; item += gridDim.x * WAVES) {
        const int e = item / HALVES, h = item % HALVES;
        const cplx* twf = LOGN == 11 ? tw + xfft::XTw2::F + h * xfft::XTw2::FH : tw;       // this half's forward tables (laid out as XTw's F1 / F2 / F3)
        cplx w1[7];
#pragma unroll
        for (int t = 0; t < 7; t++) w1[t] = twf[xfft::XTw::F1 + t];
        const int32_t* src = a.w + (size_t)e * N;
        double re[1][R], im[1][R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            if constexpr (LOGN == 11) {      // t = z_j +- c z_{j+512}: (zr, zi) = coefficients (j, j + 1024), (zr2, zi2) = (j + 512, j + 1536); int32 differences in FP64: exact
                const double c_s = h ? -xfft::SQRT_HALF : xfft::SQRT_HALF;
                const double v0 = (double)src[lane + 64 * m], v1 = (double)src[lane + 64 * m + P], v2 = (double)src[lane + 64 * m + 2 * P], v3 = (double)src[lane + 64 * m + 3 * P];
                re[0][m] = __builtin_fma(c_s, v1 - v3, v0);
                im[0][m] = __builtin_fma(c_s, v1 + v3, v2);
            } else {
                re[0][m] = (double)src[lane + 64 * m];
                im[0][m] = (double)src[lane + 64 * m + P];
            }
        }
        xfft::forward_multi_t<1>(re, im, twf + xfft::XTw::F2, twf + xfft::XTw::F3, w1, xbuf, xbuf + G::XSLOTS, lane);
        cplx* dst = a.spec + (size_t)item * P + lane;
#pragma unroll
        for (int m = 0; m < R; m++) dst[m * 64] = make_double2(re[0][m], im[0][m]);
    }
}

// ---- the product ----
struct PlainMulArgs {
    const cplx* xtw;
    const cplx* spec;          // the plain set's spectra (PlainBuildArgs)
    const int32_t* w_idx;      // [count][K], or null: entry k
    const uint32_t* x;         // [n_x][2][N]
    const int32_t* x_idx;      // [count][K], or null: row g * K + k
    uint32_t* out;             // [count][2][N]
    int32_t* fault;            // set to 1 when a sample was skipped for an out-of-range index
    int32_t count, K, n_w, n_x, accumulate;
};

// term k of sample g: the weight polynomial and the row of x it multiplies.  Wave-uniform (scalar loads).
__device__ __forceinline__ int plain_w_index(const PlainMulArgs& a, int g, int k) { return a.w_idx ? a.w_idx[(size_t)g * a.K + k] : k; }
__device__ __forceinline__ int plain_x_index(const PlainMulArgs& a, int g, int k) { return a.x_idx ? a.x_idx[(size_t)g * a.K + k] : g * a.K + k; }
// every index of sample g in range?  false: the sample is skipped
__device__ __forceinline__ bool plain_indices_ok(const PlainMulArgs& a, int g) {
    bool ok = a.K >= 1 && a.K <= PLAIN_K_MAX;
    for (int k = 0; ok && k < a.K; k++)
        ok = (unsigned)plain_w_index(a, g, k) < (unsigned)a.n_w && (unsigned)plain_x_index(a, g, k) < (unsigned)a.n_x;
    return ok;
}

// the split of a ciphertext word into signed 16-bit halves, as k_xbk_build splits a key word: lo in [-2^15, 2^15), hi in [-2^15, 2^15]
__device__ __forceinline__ void plain_split(uint32_t v, int32_t& hi, int32_t& lo) {
    const int32_t s = (int32_t)v;
    lo = (int32_t)(int16_t)s;
    hi = (int32_t)(((int64_t)s - lo) >> 16);
}

// N = 1024: one wave per (sample, polynomial)
__device__ __forceinline__ void plain_mul_wave(const PlainMulArgs& a) {
    typedef Geo<10> G;
    constexpr int N = G::N, P = G::P, R = G::R, WAVES = PLAIN_WAVES;
    static_assert(R == xfft::R && P == 512, "512-point wave transforms");
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int idx = tid; idx < xfft::XTw::TOTAL; idx += 64 * WAVES) tw[idx] = a.xtw[idx];
    cplx w1[7];       // forward pass 1: wave-uniform twiddles (scalar loads)
#pragma unroll
    for (int e = 0; e < 7; e++) w1[e] = a.xtw[xfft::XTw::F1 + e];
    __syncthreads();
    // work item = (sample, polynomial of the row); nothing below waits for another wave
    const int item = blockIdx.x * WAVES + wave;
    const int g = item >> 1, comp = item & 1;
    if (g >= a.count) return;
    if (!plain_indices_ok(a, g)) { if (a.fault && lane == 0) *a.fault = 1; return; }
    double* xbuf = reinterpret_cast<double*>(smem + (size_t)xfft::XTw::TOTAL * sizeof(cplx)) + (size_t)wave * 2 * G::XSLOTS;

    double sre[2][R], sim[2][R];       // the running spectra, [0]: hi, [1]: lo
#pragma unroll
    for (int half = 0; half < 2; half++)
#pragma unroll
        for (int m = 0; m < R; m++) { sre[half][m] = 0.0; sim[half][m] = 0.0; }
#pragma unroll 1
    for (int k = 0; k < a.K; k++) {
        const uint32_t* src = a.x + ((size_t)plain_x_index(a, g, k) * 2 + comp) * N + lane;
        double xr[2][R], xim[2][R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            int32_t h0, l0, h1, l1;
            plain_split(src[64 * m], h0, l0);
            plain_split(src[64 * m + P], h1, l1);
            xr[0][m] = (double)h0; xim[0][m] = (double)h1;
            xr[1][m] = (double)l0; xim[1][m] = (double)l1;
        }
        xfft::forward_multi<2>(xr, xim, tw, w1, xbuf, xbuf + G::XSLOTS, lane);
        const cplx* row = a.spec + (size_t)plain_w_index(a, g, k) * P + lane;
        cplx b[R];
#pragma unroll
        for (int m = 0; m < R; m++) b[m] = row[m * 64];
        xfft::mac<false>(sre[0], sim[0], b, xr[0], xim[0]);
        xfft::mac<false>(sre[1], sim[1], b, xr[1], xim[1]);
    }
    // the old row, when accumulating, is fetched under the inverse transforms
    uint32_t* o = a.out + ((size_t)g * 2 + comp) * N + lane;
    uint32_t old[2 * R];
#pragma unroll
    for (int mm = 0; mm < 2 * R; mm++) old[mm] = a.accumulate ? o[64 * mm] : 0u;
    xfft::inverse_multi<2>(sre, sim, tw, xbuf, xbuf + G::XSLOTS, lane);
#pragma unroll
    for (int m = 0; m < R; m++) {
        o[64 * m] = old[m] + xfft::rounded_hi16(sre[0][m]) + xfft::rounded_u32(sre[1][m]);
        o[64 * m + P] = old[R + m] + xfft::rounded_hi16(sim[0][m]) + xfft::rounded_u32(sim[1][m]);
    }
}

// N = 2048: a workgroup of two waves per (sample, polynomial)
__device__ __forceinline__ void plain_mul_halves(const PlainMulArgs& a) {
    typedef Geo<10> G;
    typedef xfft::XTw2 T2;
    constexpr int N = 2048, P = 512, R = 8;
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int h = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int idx = tid; idx < T2::TOTAL; idx += 128) tw[idx] = a.xtw[idx];
    __syncthreads();
    const cplx* twf = tw + T2::F + h * T2::FH;
    cplx w1[7];
#pragma unroll
    for (int e = 0; e < 7; e++) w1[e] = twf[xfft::XTw::F1 + e];
    const double c_s = h ? -xfft::SQRT_HALF : xfft::SQRT_HALF;     // stage 1: +- c, c = (1 + i) / sqrt 2
    double* xbuf = reinterpret_cast<double*>(smem + (size_t)T2::TOTAL * sizeof(cplx)) + (size_t)h * 2 * G::XSLOTS;
    cplx* trade = reinterpret_cast<cplx*>(smem + (size_t)T2::TOTAL * sizeof(cplx) + (size_t)2 * 2 * G::XSLOTS * sizeof(double));     // [2 waves][2 sums][4][64]
    // workgroup = (sample, polynomial of the row): grid = 2 * count; both waves take the same way through the barriers below
    const int g = blockIdx.x >> 1, comp = blockIdx.x & 1;
    if (g >= a.count) return;
    if (!plain_indices_ok(a, g)) { if (a.fault && tid == 0) *a.fault = 1; return; }

    double sre[2][R], sim[2][R];       // this half of the two running spectra, [0]: hi, [1]: lo
#pragma unroll
    for (int half = 0; half < 2; half++)
#pragma unroll
        for (int m = 0; m < R; m++) { sre[half][m] = 0.0; sim[half][m] = 0.0; }
#pragma unroll 1
    for (int k = 0; k < a.K; k++) {
        const uint32_t* src = a.x + ((size_t)plain_x_index(a, g, k) * 2 + comp) * N + lane;
        double xr[2][R], xim[2][R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            int32_t hi[4], lo[4];
#pragma unroll
            for (int e = 0; e < 4; e++) plain_split(src[64 * m + P * e], hi[e], lo[e]);      // coefficients j, j + 512, j + 1024, j + 1536 (j = lane + 64 m)
            xr[0][m] = __builtin_fma(c_s, (double)(hi[1] - hi[3]), (double)hi[0]); xim[0][m] = __builtin_fma(c_s, (double)(hi[1] + hi[3]), (double)hi[2]);
            xr[1][m] = __builtin_fma(c_s, (double)(lo[1] - lo[3]), (double)lo[0]); xim[1][m] = __builtin_fma(c_s, (double)(lo[1] + lo[3]), (double)lo[2]);
        }
        xfft::forward_multi_t<2>(xr, xim, twf + xfft::XTw::F2, twf + xfft::XTw::F3, w1, xbuf, xbuf + G::XSLOTS, lane);
        const cplx* row = a.spec + ((size_t)plain_w_index(a, g, k) * 2 + h) * P + lane;
        cplx b[R];
#pragma unroll
        for (int m = 0; m < R; m++) b[m] = row[m * 64];
        xfft::mac<false>(sre[0], sim[0], b, xr[0], xim[0]);
        xfft::mac<false>(sre[1], sim[1], b, xr[1], xim[1]);
    }
    // the old words of this wave's share of the row, when accumulating, are fetched under the inverse transforms
    uint32_t* o = a.out + ((size_t)g * 2 + comp) * N + lane;
    uint32_t old[4][4];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int e = 0; e < 4; e++) old[k][e] = a.accumulate ? o[64 * (4 * h + k) + P * e] : 0u;
    xfft::inverse_core<2>(sre, sim, tw + T2::I2, tw + T2::I3, xbuf, xbuf + G::XSLOTS, lane);
    // the tenth inverse stage across the halves, fused with the untwist and the rounding (k_external_product_xfft2): wave h keeps q = lane + 64 m
    // for m in [4 h, 4 h + 4) and sends the other four points of each sum to its sibling
#pragma unroll
    for (int sm = 0; sm < 2; sm++)
#pragma unroll
        for (int k = 0; k < 4; k++)
            trade[((h * 2 + sm) * 4 + k) * 64 + lane] = make_double2(h ? sre[sm][k] : sre[sm][4 + k], h ? sim[sm][k] : sim[sm][4 + k]);
    __syncthreads();
    uint32_t add[4][4];
#pragma unroll
    for (int sm = 0; sm < 2; sm++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const cplx oth = trade[(((1 - h) * 2 + sm) * 4 + k) * 64 + lane];
            const cplx uu = tw[T2::UV + ((h * 2 + 0) * 4 + k) * 64 + lane], vv = tw[T2::UV + ((h * 2 + 1) * 4 + k) * 64 + lane];
            const double tr = h ? oth.x : sre[sm][k], ti = h ? oth.y : sim[sm][k];
            const double br = h ? sre[sm][4 + k] : oth.x, bi = h ? sim[sm][4 + k] : oth.y;
            // y_q = T U + B V, y_{q+512} = (T U - B V) e^{-i pi/4}  (+ MAGIC: rounding by the addition, as untwist_round)
            const double y0r = __builtin_fma(tr, uu.x, __builtin_fma(-ti, uu.y, __builtin_fma(br, vv.x, __builtin_fma(-bi, vv.y, xfft::MAGIC))));
            const double y0i = __builtin_fma(tr, uu.y, __builtin_fma(ti, uu.x, __builtin_fma(br, vv.y, __builtin_fma(bi, vv.x, xfft::MAGIC))));
            const double dr = __builtin_fma(tr, uu.x, __builtin_fma(-ti, uu.y, __builtin_fma(-br, vv.x, bi * vv.y)));
            const double di = __builtin_fma(tr, uu.y, __builtin_fma(ti, uu.x, __builtin_fma(-br, vv.y, -(bi * vv.x))));
            const double y1r = __builtin_fma(xfft::SQRT_HALF, dr, __builtin_fma(xfft::SQRT_HALF, di, xfft::MAGIC));
            const double y1i = __builtin_fma(xfft::SQRT_HALF, di, __builtin_fma(-xfft::SQRT_HALF, dr, xfft::MAGIC));
            if (sm == 0) {
                add[k][0] = xfft::rounded_hi16(y0r); add[k][1] = xfft::rounded_hi16(y1r); add[k][2] = xfft::rounded_hi16(y0i); add[k][3] = xfft::rounded_hi16(y1i);
            } else {
                add[k][0] += xfft::rounded_u32(y0r); add[k][1] += xfft::rounded_u32(y1r); add[k][2] += xfft::rounded_u32(y0i); add[k][3] += xfft::rounded_u32(y1i);
            }
        }
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int e = 0; e < 4; e++) o[64 * (4 * h + k) + P * e] = old[k][e] + add[k][e];
}

template <int LOGN>
__global__ __launch_bounds__(LOGN == 11 ? 128 : 64 * PLAIN_WAVES, 1) void k_trlwe_mul_plain(const PlainMulArgs a) {
    static_assert(LOGN == 10 || LOGN == 11, "N = 1024 or 2048");
    if constexpr (LOGN == 11) plain_mul_halves(a);
    else plain_mul_wave(a);
}

}  // namespace rtfhe
