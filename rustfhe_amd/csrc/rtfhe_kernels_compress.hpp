// rtfhe_kernels_compress.hpp -- compressed results (include/rtfhe.h: rtfhe_tlwe_compress_batch_dev, rtfhe_trlwe_compress_batch_dev): every word of
// a result row rounded to its top k bits and the k-bit values packed into a little-endian bit stream, W = ceil(L k / 32) words per row.
//
// A row is L = L0 + P values: L0 contiguous words at `seg` of its input row, then P words gathered from `gat` of the same input row at coef[0 .. P).
//   lvl0:   the input row is the sample, n + 1 words: seg = 0, L0 = n + 1, P = 0
//   TRLWE:  the input row is [2][N], b then a:        seg = N (the a polynomial), L0 = N, gat = 0 (the b polynomial), coef = the kept coefficients
// Value i is r = ((v + 2^(31-k)) mod 2^32) >> (32 - k) (k = 32: v itself); bit j of it is stream bit i k + j, and stream bit s is bit s mod 32 of
// word s / 32 of the row's output.
//
// One lane per OUTPUT word.  Word w covers stream bits [32 w, 32 w + 32), i.e. values floor(32 w / k) .. floor((32 w + 31) / k), cut at L - 1: at
// most 17 of them at k = 2, at most 5 for k >= 8.  The lane rounds them, shifts each into place -- the first one down by the bits that belong to
// the word before, the others up -- and issues ONE plain store, so a wave writes 256 contiguous bytes and no two lanes ever touch the same word:
// no atomics, no LDS, and the bits of the last word past L k stay zero because no value is shifted into them.  A wave reads the 64 * 32 / k
// contiguous input words under its 64 output words (820 bytes at k = 10); neighbouring lanes' reads overlap by at most one word and the wave's
// loads fall into the same few 128-byte lines, which the vector L1 serves.
//
// A launch carries up to COMPRESS_COEF_MAX coefficients in its arguments and owns the values [v0, v1) of every row, v0 a multiple of 32: 32 values
// are k whole words, so a launch owns whole output words -- words [v0 k / 32, ceil(v1 k / 32)) -- and a long list is several launches.
#pragma once

#include "rtfhe_kernels.hpp"

namespace rtfhe {

constexpr int COMPRESS_COEF_MAX = 512;      // gathered values one k_compress_rows launch carries in its arguments (a multiple of 32)
constexpr int COMPRESS_THREADS = 256;

struct CompressArgs {
    const uint32_t* in;      // [count][in_stride]
    uint32_t* out;           // [count][W]
    uint32_t in_stride;      // words of an input row
    uint32_t seg, gat;       // word offsets inside an input row: the contiguous values, the polynomial the gathered ones are read from
    uint32_t L0, L;          // contiguous values, all values (L0 + P)
    uint32_t k;              // 2 .. 32
    uint32_t W;              // words of an output row: ceil(L k / 32)
    uint32_t w0, nw;         // this launch writes words [w0, w0 + nw) of every row: the values [v0, v1)
    uint32_t p0;             // coef[] starts at the first gathered value among them: value i >= L0 reads gat[coef[i - L0 - p0]]
    uint32_t total;          // lanes: count * nw (< 2^31)
    int32_t coef[COMPRESS_COEF_MAX];     // each in [0, N)
};

// grid: ceil(total / COMPRESS_THREADS) workgroups; lane t writes word w0 + t % nw of row t / nw
__global__ __launch_bounds__(COMPRESS_THREADS) void k_compress_rows(const CompressArgs a) {
    const uint32_t t = blockIdx.x * (uint32_t)COMPRESS_THREADS + threadIdx.x;      // total < 2^31: no wrap
    if (t >= a.total) return;
    const uint32_t g = t / a.nw, w = a.w0 + (t - g * a.nw);
    const uint32_t* row = a.in + (size_t)g * a.in_stride;
    const uint32_t k = a.k, sh = 32u - k, half = k < 32u ? 1u << (31u - k) : 0u;
    const uint32_t s0 = 32u * w;                                                   // w < W <= L <= 2 N = 4096: bit numbers stay far below 2^32
    const uint32_t i0 = s0 / k;
    uint32_t i1 = (s0 + 31u) / k;
    if (i1 >= a.L) i1 = a.L - 1u;                                                  // (the last word of the row alone; a launch ends on a word boundary)
    auto value = [&](uint32_t i) { return i < a.L0 ? row[a.seg + i] : row[a.gat + (uint32_t)a.coef[i - a.L0 - a.p0]]; };
    auto placed = [&](uint32_t i, uint32_t v) {
        const uint32_t r = (v + half) >> sh;
        const int off = (int)(i * k) - (int)s0;                                    // where bit 0 of r sits in this word: -(k - 1) .. 31
        return off < 0 ? r >> (uint32_t)(-off) : r << (uint32_t)off;
    };
    uint32_t word = 0;
    if (k >= 8u) {      // at most five values: all five loads are issued before the first is used (a value past i1 re-reads i1 and is dropped)
        uint32_t v[5];
#pragma unroll
        for (uint32_t e = 0; e < 5; e++) v[e] = value(i0 + e < i1 ? i0 + e : i1);
#pragma unroll
        for (uint32_t e = 0; e < 5; e++)
            if (i0 + e <= i1) word |= placed(i0 + e, v[e]);
    } else {
        for (uint32_t i = i0; i <= i1; i++) word |= placed(i, value(i));
    }
    a.out[(size_t)g * a.W + w] = word;
}

}  // namespace rtfhe
