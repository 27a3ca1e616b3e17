// rtfhe_compress_plan.cpp -- host only: compressed results (rtfhe_compress_plan.h; include/rtfhe.h, "compressed results").  The argument checks
// that rtfhe_tlwe_compress_batch_dev / rtfhe_trlwe_compress_batch_dev (rtfhe_compress.hip) run before they launch anything, the row size, and the
// key holder's CPU forms: rtfhe_tlwe_compress / _expand and rtfhe_trlwe_compress / _expand, which take a plain n or N and no context.  The
// coefficient list of the TRLWE form is rtfhe_extract_plan's (rtfhe_extract_plan.cpp), called here and not restated.  The device-side expansion
// (rtfhe_tlwe_expand_batch_dev / rtfhe_trlwe_expand_batch_dev) runs the same checks with RTFHE_COMPRESS_EXPAND and takes its inverse map of the
// coefficient list from rtfhe_expand_inverse_map.
#include "rtfhe_compress_plan.h"

#include <vector>

#include "rtfhe_extract_plan.h"
#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

namespace {

// k in range, count * L < 2^31, and the full rows [count][full_words] against the packed rows [count][W(L, k)]
int size_and_overlap(int32_t dir, int32_t k, size_t L, size_t full_words, size_t count, const void* in, const void* out, char* err, size_t err_len) {
    if (k < 2 || k > 32) return refuse(err, err_len, "k = " + num(k) + " is outside [2, 32]");
    if (!count_fits(count, L)) return refuse(err, err_len, "count * L too large (count * " + num((long long)L) + " words must be below 2^31)");
    const size_t packed_bytes = count * rtfhe_compressed_words(L, k) * 4, full_bytes = count * full_words * 4;
    const size_t in_bytes = dir == RTFHE_COMPRESS_PACK ? full_bytes : packed_bytes, out_bytes = dir == RTFHE_COMPRESS_PACK ? packed_bytes : full_bytes;
    if (rows_overlap(in, in_bytes, out, out_bytes)) return refuse(err, err_len, "the output overlaps the input rows");
    return 0;
}

// value i of a row: L0 contiguous words, then P words gathered from `gat` at idx[0 .. P)
inline uint32_t round_k(uint32_t v, int32_t k) { return k == 32 ? v : (uint32_t)(v + (1u << (31 - k))) >> (32 - k); }

void pack_row(const uint32_t* seg, size_t L0, const uint32_t* gat, const int32_t* idx, size_t P, int32_t k, uint32_t* out) {
    uint64_t acc = 0;      // the stream's bits not yet stored: fewer than 32 between values
    int bits = 0;
    for (size_t i = 0; i < L0 + P; i++) {
        acc |= (uint64_t)round_k(i < L0 ? seg[i] : gat[idx[i - L0]], k) << bits;
        bits += k;
        if (bits >= 32) { *out++ = (uint32_t)acc; acc >>= 32; bits -= 32; }
    }
    if (bits) *out = (uint32_t)acc;      // the last word: its unused high bits are zero
}

// value i of a packed row, back at the top of its word
inline uint32_t value_at(const uint32_t* row, size_t i, int32_t k) {
    const size_t s = i * (size_t)k, w = s >> 5;
    const int o = (int)(s & 31);
    uint32_t x = row[w] >> o;
    if (o + k > 32) x |= row[w + 1] << (32 - o);
    return x << (32 - k);
}

}  // namespace

extern "C" {

size_t rtfhe_compressed_words(size_t L, int32_t k) { return k < 2 || k > 32 ? 0 : (L * (size_t)k + 31) / 32; }

int rtfhe_tlwe_compress_plan(int32_t dir, int32_t n, int32_t k, size_t count, const void* in, const void* out, char* err, size_t err_len) {
    begin(err, err_len);
    if (!in || !out) return refuse(err, err_len, "null argument");
    if (n < 1) return refuse(err, err_len, "n = " + num(n) + " is below 1");
    return size_and_overlap(dir, k, (size_t)n + 1, (size_t)n + 1, count, in, out, err, err_len);
}

int rtfhe_trlwe_compress_plan(int32_t dir, int32_t N, int32_t k, int32_t P, const int32_t* coef, int32_t stride, size_t count, const void* in,
                              const void* out, int32_t* idx, char* err, size_t err_len) {
    begin(err, err_len);
    if (!in || !out || !idx) return refuse(err, err_len, "null argument");
    if (N < 1) return refuse(err, err_len, "N = " + num(N) + " is below 1");
    // the list alone: with count = 0 rtfhe_extract_plan has no size and no overlap left to look at
    if (int rc = rtfhe_extract_plan(N, P, coef, stride, 0, in, out, 0, idx, err, err_len)) return rc;
    return size_and_overlap(dir, k, (size_t)N + (size_t)P, 2 * (size_t)N, count, in, out, err, err_len);
}

int rtfhe_expand_inverse_map(int32_t N, int32_t P, const int32_t* idx, int16_t* inv) {
    if (!idx || !inv || N < 1 || N > 32768 || P < 1 || P > N) return RTFHE_ERR_INVALID;
    for (int32_t p = 0; p < P; p++)
        if (idx[p] < 0 || idx[p] >= N) return RTFHE_ERR_INVALID;
    for (int32_t j = 0; j < N; j++) inv[j] = -1;
    for (int32_t p = 0; p < P; p++) inv[idx[p]] = (int16_t)p;      // in list order: the later entry wins
    return 0;
}

int rtfhe_tlwe_compress(int32_t n, int32_t k, const uint32_t* in, uint32_t* out, size_t count) {
    if (int rc = rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, n, k, count, in, out, nullptr, 0)) return rc;
    const size_t L = (size_t)n + 1, W = rtfhe_compressed_words(L, k);
    for (size_t g = 0; g < count; g++) pack_row(in + g * L, L, nullptr, nullptr, 0, k, out + g * W);
    return 0;
}

int rtfhe_tlwe_expand(int32_t n, int32_t k, const uint32_t* in, uint32_t* out, size_t count) {
    if (int rc = rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_EXPAND, n, k, count, in, out, nullptr, 0)) return rc;
    const size_t L = (size_t)n + 1, W = rtfhe_compressed_words(L, k);
    for (size_t g = 0; g < count; g++)
        for (size_t i = 0; i < L; i++) out[g * L + i] = value_at(in + g * W, i, k);
    return 0;
}

int rtfhe_trlwe_compress(int32_t N, int32_t k, int32_t P, const int32_t* coef, int32_t stride, const uint32_t* in, uint32_t* out, size_t count) {
    std::vector<int32_t> idx(N >= 1 && P >= 1 && P <= N ? (size_t)P : 1);
    if (int rc = rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_PACK, N, k, P, coef, stride, count, in, out, idx.data(), nullptr, 0)) return rc;
    const size_t W = rtfhe_compressed_words((size_t)N + (size_t)P, k);
    for (size_t g = 0; g < count; g++) {
        const uint32_t* b = in + g * 2 * (size_t)N;
        pack_row(b + N, (size_t)N, b, idx.data(), (size_t)P, k, out + g * W);
    }
    return 0;
}

int rtfhe_trlwe_expand(int32_t N, int32_t k, int32_t P, const int32_t* coef, int32_t stride, const uint32_t* in, uint32_t* out, size_t count) {
    std::vector<int32_t> idx(N >= 1 && P >= 1 && P <= N ? (size_t)P : 1);
    if (int rc = rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_EXPAND, N, k, P, coef, stride, count, in, out, idx.data(), nullptr, 0)) return rc;
    const size_t W = rtfhe_compressed_words((size_t)N + (size_t)P, k);
    for (size_t g = 0; g < count; g++) {
        const uint32_t* row = in + g * W;
        uint32_t* b = out + g * 2 * (size_t)N;
        for (size_t i = 0; i < (size_t)N; i++) { b[i] = 0; b[(size_t)N + i] = value_at(row, i, k); }
        for (size_t p = 0; p < (size_t)P; p++) b[idx[p]] = value_at(row, (size_t)N + p, k);      // duplicates: the later entry wins
    }
    return 0;
}

}  // extern "C"
