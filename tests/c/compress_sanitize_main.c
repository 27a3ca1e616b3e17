/* Walks the host-only part of compressed results (rustfhe_amd/csrc/rtfhe_compress_plan.cpp: the argument checks of
 * rtfhe_tlwe_compress_batch_dev / rtfhe_trlwe_compress_batch_dev and the CPU twins rtfhe_tlwe_compress / _expand, rtfhe_trlwe_compress / _expand;
 * the coefficient list comes from rtfhe_extract_plan.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed.  Every
 * buffer the twins read or write is allocated at exactly the size the header promises, so that an access one word past a ragged row is caught;
 * the buffers of the refused calls are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_compress_plan.h"

static char err[200];
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

static uint32_t *words(size_t n) {      /* exactly n words (n = 0: one byte, so that the pointer is not null) */
    uint32_t *p = malloc(n ? n * 4 : 1);
    CHECK(p);
    return p;
}

/* |a - b| mod 2^32 <= lim */
static int near(uint32_t a, uint32_t b, uint32_t lim) { const uint32_t d = a - b; return d <= lim || (uint32_t)(0u - d) <= lim; }

static const int32_t KS[6] = {2, 5, 12, 16, 31, 32};

static void walk_tlwe(int32_t n, size_t count) {
    const size_t L = (size_t)n + 1;
    for (int t = 0; t < 6; t++) {
        const int32_t k = KS[t];
        const size_t W = rtfhe_compressed_words(L, k);
        CHECK(W == (L * (size_t)k + 31) / 32);
        uint32_t *x = words(count * L), *c = words(count * W), *y = words(count * L);
        for (size_t i = 0; i < count * L; i++) x[i] = rnd();
        x[0] = 0xFFFFFFFFu; x[count * L - 1] = 0xFFFFFFFFu;                         /* rounds up and wraps, first and last value */
        memset(c, 0x5A, count * W * 4);
        CHECK(rtfhe_tlwe_compress(n, k, x, c, count) == 0);
        const size_t pad = W * 32 - L * (size_t)k;
        for (size_t g = 0; g < count; g++) CHECK(pad == 0 || (c[g * W + W - 1] >> (32 - pad)) == 0);
        CHECK(rtfhe_tlwe_expand(n, k, c, y, count) == 0);
        for (size_t i = 0; i < count * L; i++) CHECK(near(y[i], x[i], k == 32 ? 0u : 1u << (31 - k)));
        CHECK(k == 32 || (y[0] == 0 && y[count * L - 1] == 0));
        free(x); free(c); free(y);
    }
}

static void walk_trlwe(int32_t N, int32_t P, const int32_t *coef, int32_t stride, size_t count) {
    const size_t L = (size_t)N + (size_t)P;
    for (int t = 0; t < 6; t++) {
        const int32_t k = KS[t];
        const size_t W = rtfhe_compressed_words(L, k);
        uint32_t *x = words(count * 2 * (size_t)N), *c = words(count * W), *y = words(count * 2 * (size_t)N);
        for (size_t i = 0; i < count * 2 * (size_t)N; i++) x[i] = rnd();
        memset(c, 0x5A, count * W * 4);
        memset(y, 0x5A, count * 2 * (size_t)N * 4);
        CHECK(rtfhe_trlwe_compress(N, k, P, coef, stride, x, c, count) == 0);
        const size_t pad = W * 32 - L * (size_t)k;
        for (size_t g = 0; g < count; g++) CHECK(pad == 0 || (c[g * W + W - 1] >> (32 - pad)) == 0);
        CHECK(rtfhe_trlwe_expand(N, k, P, coef, stride, c, y, count) == 0);
        const uint32_t lim = k == 32 ? 0u : 1u << (31 - k);
        for (size_t g = 0; g < count; g++) {
            const uint32_t *xb = x + g * 2 * (size_t)N, *yb = y + g * 2 * (size_t)N;
            for (int32_t i = 0; i < N; i++) CHECK(near(yb[N + i], xb[N + i], lim));
            for (int32_t i = 0; i < N; i++) {
                int kept = 0;
                for (int32_t p = 0; p < P && !kept; p++) kept = (coef ? coef[p] : p * stride) == i;
                CHECK(kept ? near(yb[i], xb[i], lim) : yb[i] == 0);
            }
        }
        free(x); free(c); free(y);
    }
}

static void refused_tlwe(int32_t dir, int32_t n, int32_t k, size_t count, const void *in, const void *out, const char *word) {
    memset(err, 'x', sizeof err);
    CHECK(rtfhe_tlwe_compress_plan(dir, n, k, count, in, out, err, sizeof err) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

static void refused_trlwe(int32_t dir, int32_t N, int32_t k, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *in, const void *out,
                          const char *word) {
    int32_t *idx = malloc(sizeof(int32_t) * (size_t)(P >= 1 && P <= N ? P : 1));      /* as rtfhe_compress.hip sizes it */
    CHECK(idx);
    memset(err, 'x', sizeof err);
    CHECK(rtfhe_trlwe_compress_plan(dir, N, k, P, coef, stride, count, in, out, idx, err, sizeof err) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
    free(idx);
}

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
static int32_t large_idx[1];
static int large_trlwe(size_t count, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_PACK, 2048, 10, 1, NULL, 1, count, in, out, large_idx, err, sizeof err);
}
static int large_tlwe(size_t count, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, 767, 10, count, in, out, err, sizeof err);
}

int main(void) {
    enum { N = 1024, n = 635 };
    /* the twins at the ragged shapes, buffers at exact size */
    walk_tlwe(1, 1); walk_tlwe(1, 67); walk_tlwe(635, 3); walk_tlwe(767, 2);
    {
        const int32_t one[1] = {N - 1}, desc[3] = {N - 1, 0, N / 2}, dup[5] = {3, 3, N - 1, 3, 0};
        walk_trlwe(N, 1, one, 1, 2);
        walk_trlwe(N, 3, desc, 1, 3);
        walk_trlwe(N, 5, dup, 1, 2);
        walk_trlwe(N, 16, NULL, N / 16, 2);
        walk_trlwe(N, N, NULL, 1, 1);
        walk_trlwe(2048, 33, NULL, 2048 / 33, 1);
        walk_trlwe(16, 16, NULL, 1, 3);                                             /* the twins take any N >= 1 */
        walk_trlwe(1, 1, NULL, 1, 1);
    }
    CHECK(rtfhe_compressed_words(636, 1) == 0 && rtfhe_compressed_words(636, 33) == 0 && rtfhe_compressed_words(636, 10) == 199 &&
          rtfhe_compressed_words(2048, 12) == 768 && rtfhe_compressed_words(0, 12) == 0);
    /* the checks: addresses only */
    const uintptr_t base = 0x10000000;
    const void *in = AT(base), *out = AT(0x40000000);
    for (int32_t dir = RTFHE_COMPRESS_PACK; dir <= RTFHE_COMPRESS_EXPAND; dir++) {
        memset(err, 'x', sizeof err);
        CHECK(rtfhe_tlwe_compress_plan(dir, n, 10, 3, in, out, err, sizeof err) == 0 && err[0] == 0);
        CHECK(rtfhe_tlwe_compress_plan(dir, n, 10, 0, in, out, err, sizeof err) == 0);
        CHECK(rtfhe_tlwe_compress_plan(dir, n, 32, 0x7fffffff / (n + 1), in, AT(0x7000000000000000ull), err, sizeof err) == 0);      /* the largest count * L */
        refused_tlwe(dir, n, 1, 3, in, out, "k = 1");
        refused_tlwe(dir, n, 33, 3, in, out, "k = 33");
        refused_tlwe(dir, n, (int32_t)0x80000000, 3, in, out, "k = -2147483648");
        refused_tlwe(dir, 0, 10, 3, in, out, "n = 0");
        refused_tlwe(dir, n, 10, 0x7fffffff / (n + 1) + 1, in, out, "count * L");
        refused_tlwe(dir, n, 10, ~(size_t)0, in, out, "count * L");
        refused_tlwe(dir, n, 10, 3, NULL, out, "null");
        refused_tlwe(dir, n, 10, 3, in, NULL, "null");
        refused_tlwe(dir, n, 10, 3, in, in, "overlaps");
        int32_t idx[5];
        const int32_t coef[5] = {0, 5, 5, N / 2, N - 1};
        CHECK(rtfhe_trlwe_compress_plan(dir, N, 12, 5, coef, -7, 3, in, out, idx, err, sizeof err) == 0 && err[0] == 0 && !memcmp(idx, coef, sizeof coef));
        CHECK(rtfhe_trlwe_compress_plan(dir, N, 12, 2, NULL, N - 1, 3, in, out, idx, err, sizeof err) == 0 && idx[1] == N - 1);
        CHECK(rtfhe_trlwe_compress_plan(dir, N, 12, 1, NULL, 1, 0, in, out, idx, err, sizeof err) == 0);
        const int32_t neg[3] = {0, -1, 5}, big[3] = {0, 1, N};
        refused_trlwe(dir, N, 1, 1, NULL, 1, 3, in, out, "k = 1");
        refused_trlwe(dir, N, 33, 1, NULL, 1, 3, in, out, "k = 33");
        refused_trlwe(dir, N, 12, 0, NULL, 1, 3, in, out, "P = 0");
        refused_trlwe(dir, N, 12, N + 1, NULL, 1, 3, in, out, "P = 1025");
        refused_trlwe(dir, N, 12, 3, neg, 1, 3, in, out, "sample 1: coef = -1");
        refused_trlwe(dir, N, 12, 3, big, 1, 3, in, out, "sample 2: coef = 1024");
        refused_trlwe(dir, N, 12, 3, NULL, 0, 3, in, out, "stride = 0");
        refused_trlwe(dir, N, 12, 3, NULL, N / 2, 3, in, out, "sample 2: coef = 1024");
        refused_trlwe(dir, N, 12, N, NULL, 0x7fffffff, 1, in, out, "sample 1: coef = 2147483647");
        refused_trlwe(dir, N, 12, 1, NULL, 1, 0x7fffffff / (N + 1) + 1, in, out, "count * L");
        refused_trlwe(dir, N, 12, 1, NULL, 1, 3, NULL, out, "null");
        refused_trlwe(dir, N, 12, 1, NULL, 1, 3, in, NULL, "null");
        refused_trlwe(dir, N, 12, 1, NULL, 1, 3, in, in, "overlaps");
        refused_trlwe(dir, 0, 12, 1, NULL, 1, 3, in, out, "N = 0");
        CHECK(rtfhe_trlwe_compress_plan(dir, N, 12, 1, NULL, 1, 3, in, out, NULL, err, sizeof err) == RTFHE_ERR_INVALID);      /* no room for the list */
    }
    /* the edges of the overlap test: the packed rows right behind and right before the full rows do not overlap, one word closer does */
    {
        const size_t W = rtfhe_compressed_words(n + 1, 10), full = 3 * (size_t)(n + 1) * 4, packed = 3 * W * 4;
        CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, n, 10, 3, in, AT(base + full), err, sizeof err) == 0);
        CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, n, 10, 3, in, AT(base - packed), err, sizeof err) == 0);
        refused_tlwe(RTFHE_COMPRESS_PACK, n, 10, 3, in, AT(base + full - 4), "overlaps");
        refused_tlwe(RTFHE_COMPRESS_PACK, n, 10, 3, in, AT(base - packed + 4), "overlaps");
        CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_EXPAND, n, 10, 3, in, AT(base + packed), err, sizeof err) == 0);
        CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_EXPAND, n, 10, 3, in, AT(base - full), err, sizeof err) == 0);
        refused_tlwe(RTFHE_COMPRESS_EXPAND, n, 10, 3, in, AT(base + packed - 4), "overlaps");
        refused_tlwe(RTFHE_COMPRESS_EXPAND, n, 10, 3, in, AT(base - full + 4), "overlaps");
    }
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, n, 99, 3, in, out, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, n, 99, 3, in, out, NULL, 0) == RTFHE_ERR_INVALID);
    }
    /* the public twins refuse through the same checks, before they touch a buffer */
    CHECK(rtfhe_tlwe_compress(n, 1, in, (uint32_t *)(uintptr_t)0x40000000, 3) == RTFHE_ERR_INVALID);
    CHECK(rtfhe_trlwe_expand(N, 12, N + 1, NULL, 1, in, (uint32_t *)(uintptr_t)0x40000000, 3) == RTFHE_ERR_INVALID);
    {
        const size_t most_trlwe = (size_t)0x7fffffff / 2049, most_tlwe = (size_t)0x7fffffff / 768;
        const size_t trlwe[2] = {((size_t)1 << 18) + 3, most_trlwe}, tlwe[2] = {1398102 + 3, most_tlwe};
        for (int t = 0; t < 2; t++) {
            large_cases(large_trlwe, trlwe[t], trlwe[t] * 16384, trlwe[t] * 4 * rtfhe_compressed_words(2049, 10), 4, "overlaps");
            large_cases(large_tlwe, tlwe[t], tlwe[t] * 3072, tlwe[t] * 4 * rtfhe_compressed_words(768, 10), 4, "overlaps");
        }
        large_limit(large_trlwe, most_trlwe, 16384, "count * L");
        large_limit(large_tlwe, most_tlwe, 3072, "count * L");
    }
    printf("compress sanitizer walk ok\n");
    return 0;
}
