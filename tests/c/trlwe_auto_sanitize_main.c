/* Walks the host-only part of the TRLWE key switch (rustfhe_amd/csrc/rtfhe_trlwe_auto_plan.cpp: the exponent rules of a switching key, the
 * inverse exponents, the checks of rtfhe_trlwe_auto_batch[_dev] and the automorphism on the CPU) under AddressSanitizer +
 * UndefinedBehaviorSanitizer: every refusal and every accept at the limit.  No device is needed: this code runs before any HIP call.  The
 * program arrays and exponent lists are allocated at exactly the sizes the header promises, so that a read past them is caught; the two row
 * buffers are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_trlwe_auto_plan.h"

static int plan(int32_t N, int32_t n_t, const int32_t *entry, const int32_t *add, int32_t n_steps, size_t count, const void *x, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_trlwe_auto_plan(N, n_t, entry, add, n_steps, count, x, out, err, sizeof err);
}

static void refused(int32_t N, int32_t n_t, const int32_t *entry, const int32_t *add, int32_t n_steps, size_t count, const void *x, const void *out,
                    const char *word) {
    CHECK(plan(N, n_t, entry, add, n_steps, count, x, out) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

static int exps(int32_t N, const int32_t *t, int32_t n_t) {
    memset(err, 'x', sizeof err);
    return rtfhe_trlwe_auto_exponents_plan(N, t, n_t, err, sizeof err);
}

static void exps_refused(int32_t N, const int32_t *t, int32_t n_t, const char *word) {
    CHECK(exps(N, t, n_t) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
    CHECK(rtfhe_trlwe_auto_exponents_bad(N, t, n_t) != 0);
}

/* n words, heap-allocated at their exact size */
static int32_t *words(int n, int32_t fill) {
    int32_t *p = malloc(sizeof(int32_t) * (size_t)n);
    CHECK(p);
    for (int i = 0; i < n; i++) p[i] = fill;
    return p;
}

/* buffers past 4 GiB and 16 GiB, and the item rule (sanitize_kit.h: large_cases, large_limit): `count` rows of 16 KiB in and out */
static int32_t one_step[1] = {0};
static int large_rows(size_t count, const void *x, const void *out) { return plan(2048, 1, one_step, NULL, 1, count, x, out); }

int main(void) {
    enum { N = 1024 };
    const uintptr_t base = 0x10000000;
    const void *x = AT(base), *out = AT(0x40000000);                                /* far apart: a row is 8 KiB */

    /* ---- the exponent rules ---- */
    {
        int32_t *t = words(RTFHE_TRLWE_AUTO_MAX_EXPONENTS, 0);
        for (int e = 0; e < RTFHE_TRLWE_AUTO_MAX_EXPONENTS; e++) t[e] = 2 * N - 1 - 2 * e;
        CHECK(exps(N, t, RTFHE_TRLWE_AUTO_MAX_EXPONENTS) == 0 && err[0] == 0);      /* the most exponents, 2N - 1 among them */
        CHECK(rtfhe_trlwe_auto_exponents_bad(N, t, RTFHE_TRLWE_AUTO_MAX_EXPONENTS) == 0);
        CHECK(exps(N, t, 1) == 0);
        t[0] = 1;
        CHECK(exps(N, t, 1) == 0);                                                  /* t = 1, the smallest */
        CHECK(exps(2, t, 1) == 0 && exps(1 << 20, t, 1) == 0);                      /* the smallest and the largest ring */
        exps_refused(N, t, 0, "n_t = 0");
        exps_refused(N, t, -1, "n_t = -1");
        exps_refused(N, NULL, 1, "null");
        exps_refused(0, t, 1, "N = 0");
        exps_refused(N + 1, t, 1, "N = 1025");
        exps_refused(1 << 21, t, 1, "N = 2097152");
        exps_refused(-1024, t, 1, "N = -1024");
        t[0] = 2;  exps_refused(N, t, 1, "entry 0: t = 2");
        t[0] = 0;  exps_refused(N, t, 1, "entry 0: t = 0");
        t[0] = -1; exps_refused(N, t, 1, "entry 0: t = -1");
        t[0] = 2 * N + 1; exps_refused(N, t, 1, "entry 0: t = 2049");
        t[0] = (int32_t)0x80000001; exps_refused(N, t, 1, "entry 0: t = -2147483647");
        t[0] = 0x7fffffff; exps_refused(1 << 20, t, 1, "entry 0: t = 2147483647");
        t[0] = 1; t[5] = t[2];
        exps_refused(N, t, 6, "entry 5");
        CHECK(exps(N, t, 5) == 0);
        free(t);
        {
            int32_t *big = words(RTFHE_TRLWE_AUTO_MAX_EXPONENTS + 1, 0);
            for (int e = 0; e <= RTFHE_TRLWE_AUTO_MAX_EXPONENTS; e++) big[e] = 2 * e + 1;
            exps_refused(N, big, RTFHE_TRLWE_AUTO_MAX_EXPONENTS + 1, "n_t = 65");
            free(big);
        }
    }
    /* ---- the inverse exponents: t * t^-1 = 1 mod 2N for every odd t of three rings; 0 for what breaks the rules ---- */
    {
        const int32_t rings[3] = {2, 1024, 1 << 20};
        for (int r = 0; r < 3; r++) {
            const int64_t M = 2 * (int64_t)rings[r];
            for (int64_t t = 1; t < M; t += (rings[r] > 4096 ? 4098 : 2)) {
                const int32_t v = rtfhe_trlwe_auto_inverse(rings[r], (int32_t)t);
                CHECK(v >= 1 && v < M && (v & 1) && (t * v) % M == 1);
            }
            CHECK(rtfhe_trlwe_auto_inverse(rings[r], (int32_t)(M - 1)) == (int32_t)(M - 1));
        }
        CHECK(rtfhe_trlwe_auto_inverse(N, 2) == 0 && rtfhe_trlwe_auto_inverse(N, 0) == 0 && rtfhe_trlwe_auto_inverse(N, 2 * N + 1) == 0);
        CHECK(rtfhe_trlwe_auto_inverse(N, -3) == 0 && rtfhe_trlwe_auto_inverse(N + 2, 3) == 0 && rtfhe_trlwe_auto_inverse(0, 1) == 0);
    }
    /* ---- the automorphism on the CPU: exact sizes, in place, the composition, the refusals ---- */
    {
        enum { M = 16 };
        uint32_t *p = malloc(sizeof(uint32_t) * 2 * M), *q = malloc(sizeof(uint32_t) * 2 * M);
        CHECK(p && q);
        for (int i = 0; i < 2 * M; i++) p[i] = 0x9E3779B9u * (uint32_t)(i + 1);
        CHECK(rtfhe_trlwe_automorphism(M, 5, p, q, 2) == 0);
        CHECK(q[5] == p[1] && q[3] == p[7] && q[4] == 0u - p[4] && q[M + 5] == p[M + 1]);            /* 7 * 5 = 32 + 3; 4 * 5 = 16 + 4: past M, negated */
        CHECK(rtfhe_trlwe_automorphism(M, rtfhe_trlwe_auto_inverse(M, 5), q, q, 2) == 0 && memcmp(p, q, sizeof(uint32_t) * 2 * M) == 0);
        CHECK(rtfhe_trlwe_automorphism(M, 2 * M - 1, p, q, 1) == 0 && q[0] == p[0] && q[M - 1] == 0u - p[1]);
        CHECK(rtfhe_trlwe_automorphism(M, 1, p, q, 0) == 0);
        CHECK(rtfhe_trlwe_automorphism(M, 4, p, q, 1) == RTFHE_ERR_INVALID && rtfhe_trlwe_automorphism(M, 2 * M + 1, p, q, 1) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_trlwe_automorphism(M + 1, 3, p, q, 1) == RTFHE_ERR_INVALID && rtfhe_trlwe_automorphism(0, 1, p, q, 1) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_trlwe_automorphism(M, 3, NULL, q, 1) == RTFHE_ERR_INVALID && rtfhe_trlwe_automorphism(M, 3, p, NULL, 1) == RTFHE_ERR_INVALID);
        free(p); free(q);
    }
    /* ---- a call ---- */
    {
        int32_t *e1 = words(1, 0), *e16 = words(RTFHE_TRLWE_AUTO_MAX_STEPS, 0), *a16 = words(RTFHE_TRLWE_AUTO_MAX_STEPS, 1);
        int32_t *e17 = words(RTFHE_TRLWE_AUTO_MAX_STEPS + 1, 0);
        /* accepted: one step and sixteen; the last entry of the largest key; add given and NULL; count = 0, 1 and the largest; in place */
        CHECK(plan(N, 1, e1, NULL, 1, 3, x, out) == 0 && err[0] == 0);
        e16[15] = RTFHE_TRLWE_AUTO_MAX_EXPONENTS - 1; a16[3] = 0;
        CHECK(plan(N, RTFHE_TRLWE_AUTO_MAX_EXPONENTS, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 5, x, out) == 0);
        CHECK(plan(2048, 1, e1, NULL, 1, 0, x, out) == 0);
        CHECK(plan(N, 1, e1, NULL, 1, 0x7fffffff, x, AT(0x7000000000000000ull)) == 0);
        CHECK(plan(N, 1, e1, NULL, 1, 3, x, x) == 0);                                                /* exactly in place */
        CHECK(plan(N, 1, e1, NULL, 1, 0x7fffffff, x, x) == 0);
        /* out right behind the rows, and right before them, does not overlap */
        CHECK(plan(N, 1, e1, NULL, 1, 3, x, AT(base + 3 * 2 * N * 4)) == 0);
        CHECK(plan(N, 1, e1, NULL, 1, 3, x, AT(base - 3 * 2 * N * 4)) == 0);
        /* refusals: every one is terminated inside err and names what it refuses */
        refused(N, 1, NULL, NULL, 1, 1, x, out, "null");
        refused(N, 1, e1, NULL, 1, 1, NULL, out, "null");
        refused(N, 1, e1, NULL, 1, 1, x, NULL, "null");
        refused(0, 1, e1, NULL, 1, 1, x, out, "N = 0");
        refused(1000, 1, e1, NULL, 1, 1, x, out, "N = 1000");
        refused(N, 0, e1, NULL, 1, 1, x, out, "n_t = 0");
        refused(N, 65, e1, NULL, 1, 1, x, out, "n_t = 65");
        refused(N, 1, e1, NULL, 0, 1, x, out, "n_steps = 0");
        refused(N, 1, e1, NULL, -1, 1, x, out, "n_steps = -1");
        refused(N, 1, e17, NULL, RTFHE_TRLWE_AUTO_MAX_STEPS + 1, 1, x, out, "n_steps = 17");
        refused(N, 1, e1, NULL, (int32_t)0x80000000, 1, x, out, "n_steps = -2147483648");
        refused(N, RTFHE_TRLWE_AUTO_MAX_EXPONENTS - 1, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 1, x, out, "step 15: entry = 63");
        e16[15] = -1;
        refused(N, RTFHE_TRLWE_AUTO_MAX_EXPONENTS, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 1, x, out, "step 15: entry = -1");
        e16[15] = (int32_t)0x80000000;
        refused(N, RTFHE_TRLWE_AUTO_MAX_EXPONENTS, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 1, x, out, "step 15: entry = -2147483648");
        e16[15] = 0; a16[15] = 2;
        refused(N, 1, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 1, x, out, "step 15: add = 2");
        a16[15] = -1;
        refused(N, 1, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 1, x, out, "step 15: add = -1");
        a16[15] = 1;
        CHECK(plan(N, 1, e16, a16, RTFHE_TRLWE_AUTO_MAX_STEPS, 1, x, out) == 0);
        refused(N, 1, e1, NULL, 1, (size_t)1 << 31, x, AT(0x7000000000000000ull), "count");
        refused(N, 1, e1, NULL, 1, ~(size_t)0, x, AT(0x7000000000000000ull), "count");
        refused(N, 1, e1, NULL, 1, 3, x, AT(base + 4), "overlaps");
        refused(N, 1, e1, NULL, 1, 3, x, AT(base + 3 * 2 * N * 4 - 4), "overlaps");
        refused(N, 1, e1, NULL, 1, 3, x, AT(base - 3 * 2 * N * 4 + 4), "overlaps");
        refused(N, 1, e1, NULL, 1, 3, x, AT(base + 2 * N * 4), "overlaps");                          /* shifted by one whole row */
        {   /* a message longer than err is cut, not written past it; no err at all is fine too */
            char tiny[8];
            CHECK(rtfhe_trlwe_auto_plan(N, 1, e1, NULL, 0, 1, x, out, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
            CHECK(rtfhe_trlwe_auto_plan(N, 1, e1, NULL, 0, 1, x, out, NULL, 0) == RTFHE_ERR_INVALID);
            CHECK(rtfhe_trlwe_auto_exponents_plan(N, e1, 1, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
            CHECK(rtfhe_trlwe_auto_exponents_plan(N, e1, 1, NULL, 0) == RTFHE_ERR_INVALID);
        }
        free(e1); free(e16); free(a16); free(e17);
    }
    {
        const size_t rows[2] = {((size_t)1 << 18) + 3, ((size_t)1 << 20) + 4};
        for (int t = 0; t < 2; t++) large_cases(large_rows, rows[t], rows[t] * 16384, rows[t] * 16384, 4, "overlaps");
        large_limit(large_rows, 0x7fffffff, 16384, "count");
    }
    printf("trlwe auto sanitizer walk ok\n");
    return 0;
}
