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

// ---- the other direction (include/rtfhe.h: rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev) ----
// k_expand_rows mirrors k_compress_rows: one lane per OUTPUT word, here a word of a full row.  A full row is `out_stride` words: the L0 words at
// `seg` are the values 0 .. L0 - 1 of its packed row, and (TRLWE form) word j of the b polynomial, which lies at word j of the row, is value
// L0 + p for the LAST p with coef[p] = j, or 0 where no entry names j.
//   lvl0:   seg = 0, L0 = out_stride = n + 1: every lane has a value
//   TRLWE:  seg = N (the a polynomial), L0 = N, out_stride = 2 N; "the last p, or none" is arithmetic for a NULL list (stride >= 1: j is kept
//           iff j % stride == 0 and j / stride < P) and a lookup in inv[] for a list (stride == 0): inv[j - j0] is -1 or p, built on the host
//           (rtfhe_expand_inverse_map) and carried in the arguments, EXPAND_MAP_MAX entries of int16 a launch (P <= N <= 2048 fits)
// Value i is the k-bit field at stream bits [i k, i k + k) of the row's W words: with s = i k the lane loads word s / 32 and the word after it,
// takes the 64-bit concatenation down by s % 32 (0 .. 31: never a shift by 32) and the low word of that up by 32 - k (0 .. 30), which drops every
// bit above the field -- the mask -- and leaves the value at the top of the word; k = 32 moves nothing.  THE SECOND WORD'S INDEX IS CLAMPED TO
// W - 1: no packed word at index >= W of its row is ever loaded.  The clamp only bites when the field ends inside word W - 1 (i k + k <= L k <=
// 32 W), where s % 32 + k <= 32 and no bit of the second word survives the two shifts; for the same reason the padding bits of the last word past
// L k reach no result.  Packed rows are 4-byte aligned only (W may be odd): both loads are dword loads.
//
// One plain store a lane, each output word written by exactly one lane of one launch (no memset-then-scatter: duplicates in the list would race);
// a wave writes 256 contiguous bytes and reads the 8 k contiguous bytes under them.  No LDS, no atomics.
//
// A launch owns words [o0, o0 + no) of every full row.  lvl0 and a NULL list: the whole row, one launch.  With a list: the first launch owns the
// a polynomial and the EXPAND_MAP_MAX words of b before it (o0 = N - 1024: the whole row at N = 1024), each further launch the 1,024 words of b
// before that (one more at N = 2048).
//
// Indexing: count * L < 2^31 bounds the packed values, not the output: count * 2 N reaches just under 2^32 words (P small) and byte offsets pass
// 2^32 long before.  total = count * no < 2^32 fits a u32, but the lane index of the last workgroup may pass 2^32, so it is formed and compared
// in 64 bits; row offsets are size_t.
constexpr int EXPAND_MAP_MAX = 1024;       // entries of the inverse map one k_expand_rows launch carries in its arguments (2 KB)
constexpr int EXPAND_THREADS = 256;

struct ExpandArgs {
    const uint32_t* in;      // [count][W]
    uint32_t* out;           // [count][out_stride]
    uint32_t W;              // words of a packed row: ceil(L k / 32)
    uint32_t out_stride;     // words of a full row
    uint32_t seg, L0;        // words [seg, seg + L0) of a full row are values 0 .. L0 - 1; every other word j is b[j]
    uint32_t k;              // 2 .. 32
    uint32_t o0, no;         // this launch writes words [o0, o0 + no) of every full row
    uint32_t total;          // lanes: count * no (< 2^32)
    uint32_t no_rcp;         // floor(2^32 / no) (no = 1: 2^32 - 1): t / no without a division
    uint32_t P, stride;      // stride >= 1: coef[p] = p * stride (the NULL list); stride == 0: inv[]
    uint32_t j0;             // inv[] starts at b[j0]
    int16_t inv[EXPAND_MAP_MAX];     // -1, or the last p with coef[p] = j0 + index
};

// grid: ceil(total / EXPAND_THREADS) workgroups; lane t writes word o0 + t % no of row t / no
__global__ __launch_bounds__(EXPAND_THREADS) void k_expand_rows(const ExpandArgs a) {
    const uint64_t t64 = (uint64_t)blockIdx.x * (uint32_t)EXPAND_THREADS + threadIdx.x;      // may pass 2^32 in the last workgroup: 64 bits
    if (t64 >= a.total) return;
    const uint32_t t = (uint32_t)t64;
    // t / no by the host's reciprocal: q = floor(t * floor(2^32 / no) / 2^32) is g or g - 1 (t * m / 2^32 > t / no - t / 2^32 > g - 1), so one
    // correction makes it exact -- a mul_hi and a mul_lo where a per-lane division is a float reciprocal and four multiplies (3 % of the kernel's
    // time at 131,072 lvl0 rows)
    uint32_t g = __umulhi(t, a.no_rcp), r = t - g * a.no;
    if (r >= a.no) { g++; r -= a.no; }
    const uint32_t o = a.o0 + r;
    uint32_t* dst = a.out + ((size_t)g * a.out_stride + o);
    uint32_t i = o - a.seg;                                                        // the value under this word (wraps above L0 where o < seg)
    if (i >= a.L0) {                                                               // a word of b: the last p that names it, or none
        int32_t p;
        if (a.stride) {
            const uint32_t q = o / a.stride;
            p = (q * a.stride == o && q < a.P) ? (int32_t)q : -1;
        } else {
            p = a.inv[o - a.j0];                                                   // o - j0 < EXPAND_MAP_MAX: the launch's own words of b
        }
        if (p < 0) { *dst = 0u; return; }
        i = a.L0 + (uint32_t)p;
    }
    const uint32_t* row = a.in + (size_t)g * a.W;
    const uint32_t s = __umul24(i, a.k);                                           // i < L <= 2 N = 4096, k <= 32: both fit 24 bits, s < 2^17
    const uint32_t w = s >> 5, w1 = w + 1u < a.W ? w + 1u : a.W - 1u;              // the clamp: index W is never loaded
    const uint64_t cat = (uint64_t)row[w1] << 32 | row[w];
    *dst = (uint32_t)(cat >> (s & 31u)) << (32u - a.k);
}

}  // namespace rtfhe
