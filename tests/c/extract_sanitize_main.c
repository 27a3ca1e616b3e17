/* Walks the host-only part of rtfhe_trlwe_extract_batch[_dev] / rtfhe_trlwe_extract_lvl1_batch[_dev] (rustfhe_amd/csrc/rtfhe_extract_plan.cpp:
 * every argument check that needs no context) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this code runs before
 * any HIP call.  The coefficient array is allocated at exactly the size the header promises, so that a write past it is caught; the two buffers
 * are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_extract_plan.h"

/* idx has room for P entries when 1 <= P <= N and for one entry otherwise, as rtfhe_extract.hip sizes it */
static int plan(int32_t N, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *in, const void *out, size_t out_words, int32_t **idx) {
    *idx = malloc(sizeof(int32_t) * (size_t)(P >= 1 && P <= N ? P : 1));
    CHECK(*idx);
    memset(err, 'x', sizeof err);
    return rtfhe_extract_plan(N, P, coef, stride, count, in, out, out_words, *idx, err, sizeof err);
}

static void refused(int32_t N, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *in, const void *out, size_t out_words, const char *word) {
    int32_t *idx;
    CHECK(plan(N, P, coef, stride, count, in, out, out_words, &idx) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
    free(idx);
}

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
static int32_t large_idx[1];
static int large_plan(size_t count, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_extract_plan(2048, 1, NULL, 1, count, in, out, 2049, large_idx, err, sizeof err);
}

int main(void) {
    enum { N = 1024, n1 = 636 };
    const uintptr_t base = 0x10000000;                                              /* addresses only: integers, so that no pointer arithmetic leaves an object */
    const void *in = AT(base), *out = AT(0x40000000);                               /* far apart: 3 rows are 24 KiB */
    int32_t *idx;
    {   /* a list with duplicates and both ends */
        const int32_t coef[5] = {0, 5, 5, N / 2, N - 1};
        CHECK(plan(N, 5, coef, -7, 3, in, out, n1, &idx) == 0 && err[0] == 0 && !memcmp(idx, coef, sizeof coef));      /* stride is ignored */
        free(idx);
    }
    /* coef NULL: p * stride, up to a whole row and up to the last coefficient */
    CHECK(plan(N, N, NULL, 1, 1, in, out, N + 1, &idx) == 0 && idx[0] == 0 && idx[N - 1] == N - 1);
    free(idx);
    CHECK(plan(N, 16, NULL, N / 16, 1, in, out, n1, &idx) == 0 && idx[15] == 15 * (N / 16));
    free(idx);
    CHECK(plan(N, 2, NULL, N - 1, 1, in, out, n1, &idx) == 0 && idx[1] == N - 1);
    free(idx);
    CHECK(plan(2048, 1, NULL, 0x7fffffff, 1, in, out, 2049, &idx) == 0 && idx[0] == 0);      /* (P - 1) * stride = 0 whatever the stride */
    free(idx);
    CHECK(plan(N, 1, NULL, 1, 0, in, out, n1, &idx) == 0);                                    /* count = 0 */
    free(idx);
    CHECK(plan(N, 1, NULL, 1, 0x7fffffff, in, AT(0x7000000000000000ull), n1, &idx) == 0);  /* the largest count * P */
    free(idx);
    /* out right behind the rows, and right before them, does not overlap */
    CHECK(plan(N, 1, NULL, 1, 3, in, AT(base + 3 * 2 * N * 4), n1, &idx) == 0);
    free(idx);
    CHECK(plan(N, 1, NULL, 1, 3, in, AT(base - 3 * n1 * 4), n1, &idx) == 0);
    free(idx);
    /* refusals: every one is terminated inside err and names what it refuses */
    {
        const int32_t neg[3] = {0, -1, 5}, big[3] = {0, 1, N}, min[1] = {(int32_t)0x80000000};
        refused(N, 0, NULL, 1, 1, in, out, n1, "P = 0");
        refused(N, -3, NULL, 1, 1, in, out, n1, "P = -3");
        refused(N, N + 1, NULL, 1, 1, in, out, n1, "P = 1025");
        refused(N, 0x7fffffff, NULL, 1, 1, in, out, n1, "P = 2147483647");
        refused(N, 3, neg, 1, 1, in, out, n1, "sample 1: coef = -1");
        refused(N, 3, big, 1, 1, in, out, n1, "sample 2: coef = 1024");
        refused(N, 1, min, 1, 1, in, out, n1, "sample 0: coef = -2147483648");
        refused(N, 3, NULL, 0, 1, in, out, n1, "stride = 0");
        refused(N, 3, NULL, (int32_t)0x80000000, 1, in, out, n1, "stride = -2147483648");
        refused(N, 3, NULL, N / 2, 1, in, out, n1, "sample 2: coef = 1024");
        refused(N, N, NULL, 0x7fffffff, 1, in, out, n1, "sample 1: coef = 2147483647");      /* p * stride in 64 bits */
        refused(N, 1, NULL, 1, (size_t)1 << 31, in, out, n1, "count * P");
        refused(N, 5, NULL, 1, ((size_t)1 << 31) / 5 + 1, in, out, n1, "count * P");
        refused(N, 1, NULL, 1, ~(size_t)0, in, out, n1, "count * P");
        refused(N, 1, NULL, 1, 1, NULL, out, n1, "null");
        refused(N, 1, NULL, 1, 1, in, NULL, n1, "null");
        refused(N, 1, NULL, 1, 3, in, in, n1, "overlaps");
        refused(N, 1, NULL, 1, 3, in, AT(base + 3 * 2 * N * 4 - 4), n1, "overlaps");
        refused(N, 1, NULL, 1, 3, in, AT(base - 3 * n1 * 4 + 4), n1, "overlaps");
    }
    CHECK(rtfhe_extract_plan(N, 1, NULL, 1, 1, in, out, n1, NULL, err, sizeof err) == RTFHE_ERR_INVALID);      /* no room for the coefficients */
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        const int32_t neg[1] = {-1};
        idx = malloc(sizeof(int32_t));
        CHECK(idx && rtfhe_extract_plan(N, 1, neg, 1, 1, in, out, n1, idx, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_extract_plan(N, 1, neg, 1, 1, in, out, n1, idx, NULL, 0) == RTFHE_ERR_INVALID);
        free(idx);
    }
    for (size_t count = ((size_t)1 << 18) + 3; count <= ((size_t)1 << 20) + 3; count += ((size_t)1 << 20) - ((size_t)1 << 18))
        large_cases(large_plan, count, count * 16384, count * 8196, 4, "overlaps");
    large_limit(large_plan, 0x7fffffff, 16384, "count * P");
    printf("extract sanitizer walk ok\n");
    return 0;
}
