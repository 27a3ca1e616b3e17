// rtfhe_kernels_extract.hpp -- TRLWE sample extraction (include/rtfhe.h: rtfhe_trlwe_extract_batch[_dev], rtfhe_trlwe_extract_lvl1_batch[_dev]):
// chosen coefficients of TRLWEs that already exist as lvl1 samples, TRLWERep::sample_extract_index (hom_nand/src/trlwe.rs:110-121).
//
// Sample s = g P + p of a call is e = sample_extract_index(x[g], j), j = coef[p]:
//
//     e.a[c] = x.a[j - c]  for c <= j,   0 - x.a[N + j - c]  for c > j,   e.b = x.b[j]
//
// i.e. e.a[c] = +-x.a[(j - c) mod N]: the a-polynomial read DESCENDING from j, negated past the wrap.  No arithmetic beyond that sign: the
// kernel is a permuting copy, and what it must get right is the order of its stores.
//
// TILED = true writes the batch key switch's operand (ext_slot, rtfhe_kernels.hpp): tiles of 16 samples, 16 N + 16 words each, in which the four
// coefficients kk .. kk + 3 of the 64 (quarter q, sample r) rows lie together.  One workgroup per tile; lane 16 q + r of a wave owns the 16-byte
// chunk (kk / 4, q, r), so one wave store is ONE contiguous KiB, and wave w walks the N / 64 chunk rows kk / 4 = w N/64 .. of the tile in order.
// TILED = false writes natural rows [s][N + 1] (a'[0..N), b') with the same lanes and the same loads; the rows start at odd word offsets, so
// that path stores words.
//
// The source is read straight through the L2, not staged in LDS.  A lane's four words x.a[(j - c0 - e) mod N], e = 0 .. 3, are neighbours (up to
// the wrap), and the next chunk row of the same wave continues 16 bytes below, in the same 128-byte line: a line is fetched once and its other
// seven uses hit the L1.  Staging whole polynomials instead would take 4 N bytes per distinct g of a tile -- 16 of them when P = 1, 64 KiB at
// N = 1024 and 128 KiB at N = 2048 for 64 KiB / 128 KiB of output -- and every source word is used once per sample that reads it either way.
#pragma once

#include "rtfhe_kernels.hpp"

namespace rtfhe {

typedef unsigned int ex_v4u __attribute__((ext_vector_type(4)));

constexpr int EXTRACT_COEF_MAX = 512;      // coefficients one k_trlwe_extract launch carries in its arguments
constexpr int EXTRACT_WAVES = 4;           // waves of a workgroup (= of a tile)

struct TrlweExtractArgs {
    const uint32_t* trlwe;   // [count][2][N], b then a
    uint32_t* out;           // TILED: the sample buffer (ext_slot);  else [M][N+1]
    int32_t M;               // samples of the call: count * P
    int32_t P;
    int32_t p0, np;          // this launch writes the samples with p in [p0, p0 + np) (np <= EXTRACT_COEF_MAX); the others belong to other launches
    int32_t coef[EXTRACT_COEF_MAX];     // coef[p0 + k], each in [0, N)
};

// grid: one workgroup per 16 samples, ceil(M / 16); slots s >= M of the last tile are never stored to
template <int LOGN, bool TILED>
__global__ __launch_bounds__(64 * EXTRACT_WAVES) void k_trlwe_extract(const TrlweExtractArgs a) {
    constexpr int N = 1 << LOGN, ROWS = N / 16 / EXTRACT_WAVES;      // chunk rows (of 64 chunks of 4 coefficients) per wave
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t s = blockIdx.x * 16u + (uint32_t)r;               // M < 2^31: no wrap
    if (s >= (uint32_t)a.M) return;
    const uint32_t g = s / (uint32_t)a.P;
    const int k = (int)(s - g * (uint32_t)a.P) - a.p0;
    if (k < 0 || k >= a.np) return;
    const int j = a.coef[k];
    const uint32_t* xb = a.trlwe + (size_t)g * 2 * N;
    const uint32_t* xa = xb + N;
    uint32_t* tile = a.out + (size_t)blockIdx.x * (TILED ? ext_tile_words(N) : 16 * ((size_t)N + 1));
    uint32_t* row = tile + (size_t)r * (N + 1);                      // (the natural form's row of this sample)
    if (wave == 0 && q == 0) {
        if (TILED) tile[16 * N + r] = xb[j]; else row[N] = xb[j];
    }
#pragma unroll 4
    for (int i = 0; i < ROWS; i++) {
        const int kg = wave * ROWS + i, c0 = q * (N / 4) + 4 * kg;   // this chunk: coefficients c0 .. c0 + 3
        ex_v4u v;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int d = j - c0 - e;
            const uint32_t w = xa[d & (N - 1)];
            v[e] = d < 0 ? 0u - w : w;
        }
        if (TILED) {
            *reinterpret_cast<ex_v4u*>(tile + (size_t)(kg * 64 + lane) * 4) = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) row[c0 + e] = v[e];
        }
    }
}

}  // namespace rtfhe
