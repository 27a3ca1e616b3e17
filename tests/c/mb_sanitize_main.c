/* Walks the host-only part of the multi-bit blind rotation (rustfhe_amd/csrc/rtfhe_mb_plan.cpp: the key's sizes, the roots table, the point map
 * and every argument check that needs no context) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this code runs
 * before any HIP call.  The tables and the index arrays are allocated at exactly the sizes the headers promise, so that an access past them is
 * caught; the ciphertext buffers are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_mb_plan.h"

static int call(int32_t n, int32_t g, size_t count, const int32_t *idx, int32_t n_lut, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_mb_call_plan(n, g, count, idx, n_lut, in, out, err, sizeof err);
}

static void call_refused(int32_t n, int32_t g, size_t count, const int32_t *idx, int32_t n_lut, const void *in, const void *out, const char *word) {
    CHECK(call(n, g, count, idx, n_lut, in, out) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

static int key(int32_t n, int32_t N, int32_t l, int32_t g, const void *words) {
    memset(err, 'x', sizeof err);
    return rtfhe_mb_key_plan(n, N, l, g, words, err, sizeof err);
}

static void key_refused(int32_t n, int32_t N, int32_t l, int32_t g, const void *words, const char *word) {
    CHECK(key(n, N, l, g, words) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

int main(void) {
    const void *in = AT(0x10000000), *out = AT(0x4000000000ull);

    /* sizes: ragged last groups, the figures of the default parameters */
    CHECK(rtfhe_mb_group_count(635, 2) == 318 && rtfhe_mb_group_count(635, 3) == 212 && rtfhe_mb_group_count(1, 3) == 1 && rtfhe_mb_group_count(6, 3) == 2);
    CHECK(rtfhe_mb_trgsw_count(635, 2) == 952 && rtfhe_mb_trgsw_count(635, 3) == 1480);
    CHECK(rtfhe_mb_trgsw_count(1, 2) == 1 && rtfhe_mb_trgsw_count(1, 3) == 1 && rtfhe_mb_trgsw_count(2, 2) == 3 && rtfhe_mb_trgsw_count(2, 3) == 3);
    CHECK(rtfhe_mb_trgsw_count(3, 2) == 4 && rtfhe_mb_trgsw_count(3, 3) == 7 && rtfhe_mb_trgsw_count(5, 2) == 7 && rtfhe_mb_trgsw_count(5, 3) == 10);
    CHECK(rtfhe_mb_trgsw_count(7, 2) == 10 && rtfhe_mb_trgsw_count(7, 3) == 15 && rtfhe_mb_trgsw_count(0x7fffffff, 3) > 0);
    CHECK(rtfhe_mb_trgsw_count(0, 2) == -1 && rtfhe_mb_trgsw_count(5, 1) == -1 && rtfhe_mb_trgsw_count(5, 4) == -1 && rtfhe_mb_trgsw_count(-1, 2) == -1);
    CHECK(rtfhe_mb_group_count(0, 2) == -1 && rtfhe_mb_group_count(5, 0) == -1 && rtfhe_mb_group_count(5, (int32_t)0x80000000) == -1);
    {
        rtfhe_params p = {635, 1024, 10, 3, 6, 8, 2};      /* the default parameters (n, N, nbit, l, bgbit, ks_t, ks_basebit) */
        CHECK(rtfhe_mbk_words(&p, 2) == (size_t)952 * 12 * 1024 && rtfhe_mbk_words(&p, 3) == (size_t)1480 * 12 * 1024);
        CHECK(rtfhe_mbk_words(&p, 1) == 0 && rtfhe_mbk_words(&p, 4) == 0 && rtfhe_mbk_words(NULL, 2) == 0);
        p.n = 0;
        CHECK(rtfhe_mbk_words(&p, 2) == 0);
    }

    /* the tables at exactly their sizes: W[0] = 1, unit length, odd exponents that are a permutation of 1, 5, 9, ... */
    for (int32_t N = 1024; N <= 2048; N *= 2) {
        double *W = malloc(sizeof(double) * 4 * (size_t)N);
        int32_t *q = malloc(sizeof(int32_t) * (size_t)(N / 2));
        unsigned char *seen = calloc((size_t)(N / 2), 1);
        CHECK(W && q && seen);
        CHECK(rtfhe_mb_roots(N, W) == 0 && rtfhe_mb_point_exponents(N, q) == 0);
        CHECK(W[0] == 1.0 && W[1] == 0.0);
        for (int32_t t = 0; t < 2 * N; t++) {
            const double r = W[2 * t] * W[2 * t] + W[2 * t + 1] * W[2 * t + 1];
            CHECK(r > 1.0 - 1e-15 && r < 1.0 + 1e-15);
        }
        for (int32_t p = 0; p < N / 2; p++) {
            CHECK(q[p] > 0 && q[p] < 2 * N && (q[p] & 3) == 1 && !seen[q[p] >> 2]);
            seen[q[p] >> 2] = 1;
        }
        CHECK(q[0] == 1);
        free(W); free(q); free(seen);
    }
    {
        double w[4];
        int32_t q;
        CHECK(rtfhe_mb_roots(1024, NULL) == RTFHE_ERR_INVALID && rtfhe_mb_roots(0, w) == RTFHE_ERR_INVALID && rtfhe_mb_roots(-1024, w) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_mb_roots(1000, w) == RTFHE_ERR_INVALID && rtfhe_mb_roots((int32_t)0x40000000, w) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_mb_point_exponents(1024, NULL) == RTFHE_ERR_INVALID && rtfhe_mb_point_exponents(64, &q) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_mb_point_exponents(1536, &q) == RTFHE_ERR_INVALID && rtfhe_mb_point_exponents((int32_t)0x80000000, &q) == RTFHE_ERR_INVALID);
    }

    /* a key upload */
    CHECK(key(635, 1024, 3, 2, in) == 0 && err[0] == 0);
    CHECK(key(1, 2048, 3, 3, in) == 0 && key(767, 2048, 3, 3, in) == 0);
    key_refused(635, 1024, 3, 2, NULL, "null");
    key_refused(635, 1024, 3, 1, in, "g = 1");
    key_refused(635, 1024, 3, 4, in, "g = 4");
    key_refused(635, 1024, 3, (int32_t)0x80000000, in, "g = -2147483648");
    key_refused(0, 1024, 3, 2, in, "n = 0");
    key_refused(-7, 1024, 3, 2, in, "n = -7");
    key_refused(635, 512, 3, 2, in, "N = 512");
    key_refused(635, 4096, 3, 2, in, "N = 4096");
    key_refused(635, 1024, 0, 2, in, "l = 0");
    key_refused(0x7fffffff, 1024, 3, 3, in, "too many");

    /* a call: accepted forms, then every refusal, terminated inside err and naming what it refuses */
    CHECK(call(635, 2, 64, NULL, 1, in, out) == 0 && err[0] == 0);
    CHECK(call(1, 3, 0, NULL, 1, in, out) == 0);
    CHECK(call(635, 2, 0x7fffffff, NULL, 1, in, out) == 0);
    CHECK(call(635, 2, 5, NULL, 3, in, in) == 0);
    {
        int32_t *idx = malloc(sizeof(int32_t) * 5);
        CHECK(idx);
        for (int i = 0; i < 5; i++) idx[i] = i % 3;
        CHECK(call(635, 3, 5, idx, 3, in, out) == 0);
        idx[3] = 3; idx[4] = -1;
        call_refused(635, 3, 5, idx, 3, in, out, "lut_idx[3] = 3");          /* the FIRST offender */
        idx[3] = (int32_t)0x80000000;
        call_refused(635, 3, 5, idx, 3, in, out, "lut_idx[3] = -2147483648");
        CHECK(call(635, 3, 3, idx, 3, in, out) == 0);                        /* the array is read up to count only */
        call_refused(635, 3, 5, idx, 0, in, out, "n_lut = 0");               /* before the array is read */
        free(idx);
    }
    call_refused(635, 2, 5, NULL, 1, NULL, out, "null");
    call_refused(635, 2, 5, NULL, 1, in, NULL, "null");
    call_refused(635, 1, 5, NULL, 1, in, out, "g = 1");
    call_refused(635, 4, 5, NULL, 1, in, out, "g = 4");
    call_refused(635, 0, 5, NULL, 1, in, out, "g = 0");
    call_refused(0, 2, 5, NULL, 1, in, out, "n = 0");
    call_refused(635, 2, (size_t)0x80000000, NULL, 1, in, out, "count too large");
    call_refused(635, 2, ~(size_t)0, NULL, 1, in, out, "count too large");
    call_refused(635, 2, 5, NULL, -4, in, out, "n_lut = -4");
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_mb_call_plan(635, 7, 5, NULL, 1, in, out, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_mb_call_plan(635, 7, 5, NULL, 1, in, out, NULL, 0) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_mb_key_plan(635, 1024, 3, 7, in, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_mb_key_plan(635, 1024, 3, 7, in, NULL, 0) == RTFHE_ERR_INVALID);
    }
    printf("mb sanitizer walk ok\n");
    return 0;
}
