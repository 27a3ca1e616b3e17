/* Walks the host-only part of the device-side expansion of compressed rows (rtfhe_tlwe_expand_batch_dev / rtfhe_trlwe_expand_batch_dev in
 * rustfhe_amd/csrc/rtfhe_compress.hip) under AddressSanitizer + UndefinedBehaviorSanitizer: the RTFHE_COMPRESS_EXPAND checks called the way the
 * entry points call them -- the list resolved into an idx sized as they size it, then rtfhe_expand_inverse_map into exactly N int16 -- and the map
 * itself against a search and against what the CPU twin rtfhe_trlwe_expand does with the same list.  No device is needed.  Every buffer that is
 * read or written is allocated at exactly its size; the buffers of the checks are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_compress_plan.h"

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint32_t rnd(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

/* what rtfhe_trlwe_expand_batch_dev does on the host with (N, k, P, coef, stride, count) before it launches: 0 and *inv_out = the map (NULL for a
 * NULL list: the kernel computes it), or the plan's code with its message in err */
static int host_side(int32_t N, int32_t k, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *d_words, const void *d_trlwe,
                     int16_t **inv_out) {
    int32_t *idx = malloc(sizeof(int32_t) * (size_t)(P >= 1 && P <= N ? P : 1));
    CHECK(idx);
    *inv_out = NULL;
    memset(err, 'x', sizeof err);
    int rc = rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_EXPAND, N, k, P, coef, stride, count, d_words, d_trlwe, idx, err, sizeof err);
    CHECK(memchr(err, 0, sizeof err));
    if (rc == 0 && coef) {
        int16_t *inv = malloc(sizeof(int16_t) * (size_t)N);      /* exactly N entries */
        CHECK(inv);
        CHECK(rtfhe_expand_inverse_map(N, P, idx, inv) == 0);
        for (int32_t j = 0; j < N; j++) {                        /* the last p that names j, by search */
            int32_t last = -1;
            for (int32_t p = 0; p < P; p++)
                if (coef[p] == j) last = p;
            CHECK(inv[j] == last);
        }
        *inv_out = inv;
    }
    free(idx);
    return rc;
}

/* the map against the CPU twin: b[j] of the expanded row is value N + inv[j], or 0 */
static void walk_list(int32_t N, int32_t P, const int32_t *coef, int32_t k) {
    const size_t L = (size_t)N + (size_t)P, W = rtfhe_compressed_words(L, k), count = 2;
    uint32_t *full = malloc(count * 2 * (size_t)N * 4), *packed = malloc(count * W * 4), *back = malloc(count * 2 * (size_t)N * 4);
    CHECK(full && packed && back);
    for (size_t i = 0; i < count * 2 * (size_t)N; i++) full[i] = rnd();
    int16_t *inv;
    CHECK(host_side(N, k, P, coef, 1, count, AT(0x10000000), AT(0x40000000), &inv) == 0 && inv && err[0] == 0);
    /* packed rows whose kept values all differ, so that which duplicate wins shows: made from a list of distinct coefficients 0 .. P - 1 */
    CHECK(rtfhe_trlwe_compress(N, k, P, NULL, 1, full, packed, count) == 0);
    memset(back, 0x5A, count * 2 * (size_t)N * 4);
    CHECK(rtfhe_trlwe_expand(N, k, P, coef, 1, packed, back, count) == 0);
    const uint32_t half = k == 32 ? 0u : 1u << (31 - k);
    for (size_t g = 0; g < count; g++)
        for (int32_t j = 0; j < N; j++) {
            const uint32_t v = full[g * 2 * (size_t)N + (size_t)(inv[j] < 0 ? 0 : inv[j])];      /* b[inv[j]] of the source row: value N + inv[j] */
            const uint32_t want = inv[j] < 0 ? 0u : (k == 32 ? v : (uint32_t)(v + half) >> (32 - k) << (32 - k));
            CHECK(back[g * 2 * (size_t)N + (size_t)j] == want);
        }
    free(inv); free(full); free(packed); free(back);
}

static void refused(int32_t N, int32_t k, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *in, const void *out, const char *word) {
    int16_t *inv;
    CHECK(host_side(N, k, P, coef, stride, count, in, out, &inv) == RTFHE_ERR_INVALID && inv == NULL);
    CHECK(strstr(err, word));
}

static void refused_tlwe(int32_t n, int32_t k, size_t count, const void *in, const void *out, const char *word) {
    memset(err, 'x', sizeof err);
    CHECK(rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_EXPAND, n, k, count, in, out, err, sizeof err) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

/* the far outputs of tests/test_gpu_expand_large.py: the packed rows are the input, the full rows the output */
static int32_t large_idx[1];
static int large_trlwe(size_t count, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_EXPAND, 1024, 12, 1, NULL, 1, count, in, out, large_idx, err, sizeof err);
}
static int large_tlwe(size_t count, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_EXPAND, 767, 10, count, in, out, err, sizeof err);
}

int main(void) {
    enum { N = 1024, n = 635 };
    static const int32_t KS[6] = {2, 5, 12, 16, 31, 32};
    {
        int32_t *desc = malloc(sizeof(int32_t) * 2048), *rand_list = malloc(sizeof(int32_t) * 2048);
        CHECK(desc && rand_list);
        const int32_t one[1] = {N - 1}, three[3] = {N - 1, 0, N / 2}, dup[5] = {3, 3, N - 1, 3, 0}, far_dup[6] = {9, 1000, 9, 4, 1000, 9}, zero[1] = {0};
        for (int t = 0; t < 6; t++) {
            const int32_t k = KS[t];
            walk_list(N, 1, one, k);
            walk_list(N, 3, three, k);
            walk_list(N, 5, dup, k);
            walk_list(N, 6, far_dup, k);
            for (int32_t NN = 1024; NN <= 2048; NN *= 2) {
                for (int32_t p = 0; p < NN; p++) { desc[p] = NN - 1 - p; rand_list[p] = (int32_t)(rnd() % (uint32_t)NN); }
                walk_list(NN, NN, desc, k);                                          /* P = N, a whole row backwards */
                walk_list(NN, NN, rand_list, k);                                     /* P = N with many duplicates and many gaps */
                walk_list(NN, 33, rand_list, k);
            }
            walk_list(16, 16, desc + 2048 - 16, k);                                  /* the map takes any N >= 1 */
            walk_list(1, 1, zero, k);
        }
        free(desc); free(rand_list);
    }
    /* the map's own refusals leave inv alone */
    {
        int16_t inv[4] = {0x5A5A, 0x5A5A, 0x5A5A, 0x5A5A};
        const int32_t ok[2] = {1, 0}, neg[2] = {0, -1}, big[2] = {0, 4};
        CHECK(rtfhe_expand_inverse_map(4, 2, NULL, inv) == RTFHE_ERR_INVALID && rtfhe_expand_inverse_map(4, 2, ok, NULL) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_expand_inverse_map(0, 1, ok, inv) == RTFHE_ERR_INVALID && rtfhe_expand_inverse_map(32769, 1, ok, inv) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_expand_inverse_map(4, 0, ok, inv) == RTFHE_ERR_INVALID && rtfhe_expand_inverse_map(1, 2, ok, inv) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_expand_inverse_map(4, 2, neg, inv) == RTFHE_ERR_INVALID && rtfhe_expand_inverse_map(4, 2, big, inv) == RTFHE_ERR_INVALID);
        for (int j = 0; j < 4; j++) CHECK(inv[j] == 0x5A5A);
        CHECK(rtfhe_expand_inverse_map(4, 2, ok, inv) == 0 && inv[0] == 1 && inv[1] == 0 && inv[2] == -1 && inv[3] == -1);
    }
    /* the checks of both entry points: addresses only */
    const uintptr_t base = 0x10000000;
    const void *in = AT(base), *out = AT(0x40000000);
    {
        int16_t *inv;
        const int32_t neg[3] = {0, -1, 5}, big[3] = {0, 1, N};
        CHECK(host_side(N, 12, 1, NULL, 1, 3, in, out, &inv) == 0 && inv == NULL && err[0] == 0);
        CHECK(host_side(N, 12, N, NULL, 1, 0, in, out, &inv) == 0 && inv == NULL);                                /* count = 0 */
        CHECK(host_side(N, 32, 1, NULL, 1, 0x7fffffff / (N + 1), in, AT(0x7000000000000000ull), &inv) == 0);      /* the largest count * L */
        refused(N, 1, 1, NULL, 1, 3, in, out, "k = 1");
        refused(N, 33, 1, NULL, 1, 3, in, out, "k = 33");
        refused(N, 12, 0, NULL, 1, 3, in, out, "P = 0");
        refused(N, 12, N + 1, NULL, 1, 3, in, out, "P = 1025");
        refused(N, 12, 3, neg, 1, 3, in, out, "sample 1: coef = -1");
        refused(N, 12, 3, big, 1, 3, in, out, "sample 2: coef = 1024");
        refused(N, 12, 3, NULL, 0, 3, in, out, "stride = 0");
        refused(N, 12, 3, NULL, N / 2, 3, in, out, "sample 2: coef = 1024");
        refused(N, 12, 1, NULL, 1, 0x7fffffff / (N + 1) + 1, in, out, "count * L");
        refused(N, 12, 1, NULL, 1, ~(size_t)0, in, out, "count * L");
        refused(N, 12, 1, NULL, 1, 3, NULL, out, "null");
        refused(N, 12, 1, NULL, 1, 3, in, NULL, "null");
        refused(N, 12, 1, NULL, 1, 3, in, in, "overlaps");
        refused_tlwe(n, 1, 3, in, out, "k = 1");
        refused_tlwe(n, 33, 3, in, out, "k = 33");
        refused_tlwe(n, 10, 0x7fffffff / (n + 1) + 1, in, out, "count * L");
        refused_tlwe(n, 10, 3, NULL, out, "null");
        refused_tlwe(n, 10, 3, in, NULL, "null");
        refused_tlwe(n, 10, 3, in, in, "overlaps");
    }
    /* the edges of the overlap test in this direction: the input is the packed rows, the output the full rows */
    {
        const size_t W = rtfhe_compressed_words(N + 5, 12), packed = 3 * W * 4, full = 3 * 2 * (size_t)N * 4;
        int16_t *inv;
        CHECK(host_side(N, 12, 5, NULL, 1, 3, in, AT(base + packed), &inv) == 0);
        CHECK(host_side(N, 12, 5, NULL, 1, 3, in, AT(base - full), &inv) == 0);
        refused(N, 12, 5, NULL, 1, 3, in, AT(base + packed - 4), "overlaps");
        refused(N, 12, 5, NULL, 1, 3, in, AT(base - full + 4), "overlaps");
    }
    /* outputs past 4 GiB from inputs below it, and the item rule */
    {
        const size_t trlwe = 524288 + 3, tlwe = 1398102 + 3;
        large_cases(large_trlwe, trlwe, trlwe * 4 * rtfhe_compressed_words(1025, 12), trlwe * 8192, 4, "overlaps");
        large_cases(large_tlwe, tlwe, tlwe * 4 * rtfhe_compressed_words(768, 10), tlwe * 3072, 4, "overlaps");
        large_limit(large_trlwe, (size_t)0x7fffffff / 1025, 8192, "count * L");
        large_limit(large_tlwe, (size_t)0x7fffffff / 768, 3072, "count * L");
    }
    printf("expand sanitizer walk ok\n");
    return 0;
}
