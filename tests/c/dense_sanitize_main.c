/* Walks the host-only part of rtfhe_dense_create and rtfhe_tlwe_dense_batch[_dev] (rustfhe_amd/csrc/rtfhe_dense_plan.cpp: every argument check
 * that needs no context, the correction words, the launch rule) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this
 * code runs before any HIP call.  The matrices and the correction words are allocated at exactly the sizes the header promises, so that an
 * access past them is caught; the two buffers are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_dense_plan.h"

static int plan(int32_t n, int32_t O, int32_t I, size_t count, const void *x, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_dense_plan(n, O, I, count, x, out, err, sizeof err);
}

static void refused(int32_t n, int32_t O, int32_t I, size_t count, const void *x, const void *out, const char *word) {
    CHECK(plan(n, O, I, count, x, out) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

/* [O][I] weights, heap-allocated at their exact size */
static int32_t *matrix(int32_t O, int32_t I, int32_t fill) {
    int32_t *p = malloc(sizeof(int32_t) * (size_t)O * (size_t)I);
    CHECK(p);
    for (size_t i = 0; i < (size_t)O * (size_t)I; i++) p[i] = fill;
    return p;
}

static int weights(const int32_t *W, int32_t O, int32_t I, uint32_t *corr) {
    memset(err, 'x', sizeof err);
    return rtfhe_dense_weights_plan(W, O, I, corr, err, sizeof err);
}

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
static int large_plan(size_t count, const void *x, const void *out) { return plan(767, 16, 64, count, x, out); }

int main(void) {
    const uintptr_t base = 0x10000000;                                              /* addresses only: integers, so that no pointer arithmetic leaves an object */
    const void *x = AT(base), *out = AT(0x4000000000ull);

    {   /* correction words: 128 * 0x01010101 * the row sum, both signs, and the widest row */
        int32_t *W = matrix(3, 5, 0);
        uint32_t *corr = malloc(sizeof(uint32_t) * 3);
        CHECK(corr);
        W[0] = 1;                                                                   /* sum 1 */
        for (int i = 0; i < 5; i++) W[5 + i] = -128;                                /* sum -640 */
        for (int i = 0; i < 5; i++) W[10 + i] = 127;                                /* sum 635 */
        CHECK(weights(W, 3, 5, corr) == 0 && err[0] == 0);
        CHECK(corr[0] == 0x80808080u && corr[1] == (uint32_t)(0x80808080u * (uint32_t)-640) && corr[2] == (uint32_t)(0x80808080u * 635u));
        W[7] = 128;
        corr[0] = corr[1] = corr[2] = 0xAAAAAAAAu;
        CHECK(weights(W, 3, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "W[1][2] = 128") && corr[0] == 0xAAAAAAAAu);     /* nothing written on refusal */
        W[7] = -129; W[14] = 1000;
        CHECK(weights(W, 3, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "W[1][2] = -129"));                              /* the FIRST offender */
        W[7] = (int32_t)0x80000000;
        CHECK(weights(W, 3, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "W[1][2] = -2147483648"));
        CHECK(weights(NULL, 3, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "null"));
        CHECK(weights(W, 3, 5, NULL) == RTFHE_ERR_INVALID && strstr(err, "null"));
        /* the limits are checked before W is read: W holds 15 entries only */
        CHECK(weights(W, 0, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "O = 0"));
        CHECK(weights(W, 65537, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "O = 65537"));
        CHECK(weights(W, -1, 5, corr) == RTFHE_ERR_INVALID && strstr(err, "O = -1"));
        CHECK(weights(W, 3, 0, corr) == RTFHE_ERR_INVALID && strstr(err, "I = 0"));
        CHECK(weights(W, 3, 65537, corr) == RTFHE_ERR_INVALID && strstr(err, "I = 65537"));
        CHECK(weights(W, 3, (int32_t)0x80000000, corr) == RTFHE_ERR_INVALID && strstr(err, "I = -2147483648"));
        free(W); free(corr);
    }
    {   /* the widest row the interface accepts, all -128: the sum is -2^23 */
        int32_t *W = matrix(1, RTFHE_DENSE_MAX, -128);
        uint32_t corr = 0;
        CHECK(weights(W, 1, RTFHE_DENSE_MAX, &corr) == 0 && corr == (uint32_t)(0x80808080u * (uint32_t)(-(int32_t)(1 << 23))));
        free(W);
        W = matrix(RTFHE_DENSE_MAX, 1, 127);
        uint32_t *c = malloc(sizeof(uint32_t) * RTFHE_DENSE_MAX);
        CHECK(c && weights(W, RTFHE_DENSE_MAX, 1, c) == 0 && c[RTFHE_DENSE_MAX - 1] == (uint32_t)(0x80808080u * 127u));
        free(W); free(c);
    }

    /* accepted: the smallest call, the limits, count = 0, the largest word count below 2^31 */
    CHECK(plan(1, 1, 1, 1, x, out) == 0 && err[0] == 0);
    CHECK(plan(767, 65536, 65536, 42, x, out) == 0);                                 /* 42 * 65,536 * 768 = 2^31 - 2^25 ... below 2^31 */
    CHECK(plan(635, 32, 784, 0, x, out) == 0);
    CHECK(plan(635, 32, 784, 0, x, x) == 0);                                         /* count = 0: nothing to overlap */
    CHECK(plan(1, 1, 1, 0x3fffffff, x, out) == 0);                                   /* (2^30 - 1) * 1 * 2 < 2^31 */
    /* out right behind the rows, and right before them, does not overlap: x is 3 * 7 * 41 words, out 3 * 2 * 41 */
    CHECK(plan(40, 2, 7, 3, x, AT(base + 3 * 7 * 41 * 4)) == 0);
    CHECK(plan(40, 2, 7, 3, x, AT(base - 3 * 2 * 41 * 4)) == 0);
    /* refusals: every one is terminated inside err and names what it refuses */
    refused(40, 2, 7, 3, NULL, out, "null");
    refused(40, 2, 7, 3, x, NULL, "null");
    refused(0, 2, 7, 3, x, out, "n = 0");
    refused(-3, 2, 7, 3, x, out, "n = -3");
    refused(40, 0, 7, 3, x, out, "O = 0");
    refused(40, 65537, 7, 3, x, out, "O = 65537");
    refused(40, 2, 0, 3, x, out, "I = 0");
    refused(40, 2, 65537, 3, x, out, "I = 65537");
    refused(767, 65536, 1, 43, x, out, "count * max(I, O) * (n + 1)");               /* 43 * 65,536 * 768 > 2^31 */
    refused(1, 1, 1, 0x40000000, x, out, "count * max(I, O) * (n + 1)");             /* 2^30 * 2 = 2^31 */
    refused(1, 1, 1, ~(size_t)0, x, out, "count * max(I, O) * (n + 1)");
    refused(40, 2, 7, 3, x, x, "overlaps");
    refused(40, 2, 7, 3, x, AT(base + 3 * 7 * 41 * 4 - 4), "overlaps");
    refused(40, 2, 7, 3, x, AT(base - 3 * 2 * 41 * 4 + 4), "overlaps");
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_dense_plan(40, 65537, 7, 3, x, out, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_dense_plan(40, 65537, 7, 3, x, out, NULL, 0) == RTFHE_ERR_INVALID);
    }
    {   /* the launch rule: slices never empty, every K-step covered, at least two K-steps per slice when I is cut */
        static const int32_t ns[] = {1, 15, 16, 40, 635, 767}, Os[] = {1, 15, 16, 17, 33, 64, 65, 512, 65536}, Is[] = {1, 63, 64, 65, 200, 256, 784, 65536};
        static const size_t counts[] = {1, 2, 5, 256, 8192};
        for (size_t a = 0; a < sizeof ns / sizeof *ns; a++)
            for (size_t b = 0; b < sizeof Os / sizeof *Os; b++)
                for (size_t c = 0; c < sizeof Is / sizeof *Is; c++)
                    for (size_t d = 0; d < sizeof counts / sizeof *counts; d++) {
                        rtfhe_dense_shape s;
                        rtfhe_dense_launch_shape(ns[a], Os[b], Is[c], counts[d], 256, &s);
                        CHECK(s.tiles == 1 || s.tiles == 2 || s.tiles == 4);
                        CHECK(s.groups * s.tiles * 16 >= Os[b] && (s.groups - 1) * s.tiles * 16 < Os[b]);
                        CHECK(s.cwgs * 4 * 16 * RTFHE_DENSE_CT >= ns[a] + 1 && (s.cwgs - 1) * 4 * 16 * RTFHE_DENSE_CT < ns[a] + 1);
                        CHECK(s.ksteps * 64 >= Is[c] && (s.ksteps - 1) * 64 < Is[c]);
                        CHECK(s.slices >= 1 && s.slices * s.steps >= s.ksteps && (s.slices - 1) * s.steps < s.ksteps);
                        CHECK(s.slices == 1 || s.steps >= 2);
                        CHECK(s.slices == 1 || counts[d] * (size_t)s.groups * (size_t)s.cwgs < 512);
                    }
        rtfhe_dense_shape s;
        rtfhe_dense_launch_shape(40, 16, 65536, 1, 256, &s);                         /* one workgroup of work, 1,024 K-steps: 512 slices of two */
        CHECK(s.tiles == 1 && s.groups == 1 && s.cwgs == 1 && s.ksteps == 1024 && s.slices == 512 && s.steps == 2);
        rtfhe_dense_launch_shape(635, 32, 784, 1024, 256, &s);                       /* a full batch: plain stores */
        CHECK(s.tiles == 2 && s.groups == 1 && s.cwgs == 5 && s.ksteps == 13 && s.slices == 1 && s.steps == 13);
        rtfhe_dense_launch_shape(635, 32, 784, 1, 0, &s);                            /* cus below 1 counts as 1 */
        CHECK(s.slices == 1);
    }
    {
        const size_t most = (size_t)0x7fffffff / (64 * 768), counts[2] = {21900, most};
        for (int t = 0; t < 2; t++) large_cases(large_plan, counts[t], counts[t] * 64 * 3072, counts[t] * 16 * 3072, 4, "overlaps");
        large_limit(large_plan, most, 64 * 3072, "count * max(I, O)");
    }
    printf("dense sanitizer walk ok\n");
    return 0;
}
