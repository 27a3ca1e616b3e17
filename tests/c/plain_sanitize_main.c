/* Walks the host-only part of rtfhe_plain_create and rtfhe_trlwe_mul_plain_batch[_dev] (rustfhe_amd/csrc/rtfhe_plain_plan.cpp: every argument
 * check that needs no context) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this code runs before any HIP call.
 * The weight and index arrays are allocated at exactly the sizes the header promises, so that a read past them is caught; the two buffers are
 * addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_plain_plan.h"

static int plan(int32_t N, int32_t n_w, int64_t wmax, int32_t K, int32_t wg, const int32_t *w_idx, int32_t n_x, int32_t xg, const int32_t *x_idx, size_t count,
                const void *x, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_plain_plan(N, n_w, wmax, K, wg, w_idx, n_x, xg, x_idx, count, x, out, err, sizeof err);
}

static void refused(int32_t N, int32_t n_w, int64_t wmax, int32_t K, int32_t wg, const int32_t *w_idx, int32_t n_x, int32_t xg, const int32_t *x_idx,
                    size_t count, const void *x, const void *out, const char *word) {
    CHECK(plan(N, n_w, wmax, K, wg, w_idx, n_x, xg, x_idx, count, x, out) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

/* [count][K] indices, heap-allocated at their exact size */
static int32_t *indices(size_t count, int K, int32_t fill) {
    int32_t *p = malloc(sizeof(int32_t) * count * (size_t)K);
    CHECK(p);
    for (size_t i = 0; i < count * (size_t)K; i++) p[i] = fill;
    return p;
}

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
/* x of `rows` rows read by 64 samples (x_idx given: on the device), then 64 rows of x and `count` samples: the output is the far array */
static int large_x(size_t rows, const void *x, const void *out) { return plan(2048, 1, 0, 1, 0, NULL, (int32_t)rows, 1, NULL, 64, x, out); }
static int large_out(size_t count, const void *x, const void *out) { return plan(2048, 1, 0, 1, 0, NULL, 64, 1, NULL, count, x, out); }

int main(void) {
    enum { N = 1024 };
    const uintptr_t base = 0x10000000;                                              /* addresses only: integers, so that no pointer arithmetic leaves an object */
    const void *x = AT(base), *out = AT(0x40000000);                                /* far apart: a row is 8 KiB */
    const int64_t LIM = (int64_t)RTFHE_PLAIN_L1_PER_N * N;

    {   /* wmax of a set: the largest l1 norm, int32 minimum included */
        int32_t *w = calloc((size_t)3 * N, sizeof(int32_t));
        int64_t wmax = -1;
        CHECK(w);
        w[0] = 5; w[N - 1] = -7;                                                    /* 12 */
        for (int c = 0; c < N; c++) w[N + c] = (c & 1) ? -192 : 192;                /* 192 N */
        w[2 * N + 3] = (int32_t)0x80000000;                                         /* 2^31 */
        CHECK(rtfhe_plain_weights_plan(N, w, 1, &wmax, err, sizeof err) == 0 && wmax == 12);
        CHECK(rtfhe_plain_weights_plan(N, w, 2, &wmax, err, sizeof err) == 0 && wmax == LIM);
        CHECK(rtfhe_plain_weights_plan(N, w, 3, &wmax, err, sizeof err) == 0 && wmax == ((int64_t)1 << 31));
        for (int c = 0; c < N; c++) w[c] = (int32_t)0x80000000;
        CHECK(rtfhe_plain_weights_plan(N, w, 1, &wmax, err, sizeof err) == 0 && wmax == ((int64_t)N << 31));
        CHECK(rtfhe_plain_weights_plan(N, NULL, 1, &wmax, err, sizeof err) == RTFHE_ERR_INVALID && strstr(err, "null"));
        CHECK(rtfhe_plain_weights_plan(N, w, 1, NULL, err, sizeof err) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_plain_weights_plan(N, w, 0, &wmax, err, sizeof err) == RTFHE_ERR_INVALID && strstr(err, "n_w = 0"));
        CHECK(rtfhe_plain_weights_plan(N, w, -2, &wmax, err, sizeof err) == RTFHE_ERR_INVALID && strstr(err, "n_w = -2"));
        CHECK(rtfhe_plain_weights_plan(N, w, 0x7fffffff, &wmax, err, sizeof err) == RTFHE_ERR_INVALID && strstr(err, "n_w * N"));
        free(w);
    }

    /* accepted: the limit exactly, at K = 1 and at K = 8; NULL indices at their exact needs; count = 0; the largest count * K */
    CHECK(plan(N, 1, LIM, 1, 0, NULL, 3, 0, NULL, 3, x, out) == 0 && err[0] == 0);
    CHECK(plan(N, 8, LIM / 8, 8, 0, NULL, 24, 0, NULL, 3, x, out) == 0);
    CHECK(plan(2048, 8, 24 * 2048, 8, 0, NULL, 8, 0, NULL, 1, x, out) == 0);
    CHECK(plan(N, 1, 0, 1, 0, NULL, 1, 0, NULL, 0, x, out) == 0);
    CHECK(plan(N, 1, 5, 2, 0, NULL, 1, 0, NULL, 0, x, out) == 0);                                   /* count = 0: the NULL-index rules ask for nothing */
    CHECK(plan(N, 1, 1, 1, 1, NULL, 1, 1, NULL, 0x7fffffff, x, AT(0x7000000000000000ull)) == 0);  /* index arrays on the device: not walked */
    {   /* host indices with duplicates and both ends; one x row shared by all samples */
        int32_t *wi = indices(5, 3, 0), *xi = indices(5, 3, 0);
        wi[4] = 6; wi[14] = 6; xi[7] = 1; xi[14] = 1;
        CHECK(plan(N, 7, 100, 3, 1, wi, 2, 1, xi, 5, x, out) == 0);
        wi[14] = 7;
        refused(N, 7, 100, 3, 1, wi, 2, 1, xi, 5, x, out, "sample 4: w_idx[2] = 7");
        wi[14] = -1;
        refused(N, 7, 100, 3, 1, wi, 2, 1, xi, 5, x, out, "sample 4: w_idx[2] = -1");
        wi[14] = 0; xi[3] = 2;
        refused(N, 7, 100, 3, 1, wi, 2, 1, xi, 5, x, out, "sample 1: x_idx[0] = 2");
        xi[3] = (int32_t)0x80000000;
        refused(N, 7, 100, 3, 1, wi, 2, 1, xi, 5, x, out, "sample 1: x_idx[0] = -2147483648");
        free(wi); free(xi);
    }
    /* out right behind the rows, and right before them, does not overlap */
    CHECK(plan(N, 1, 1, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base + 3 * 2 * N * 4)) == 0);
    CHECK(plan(N, 1, 1, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base - 3 * 2 * N * 4)) == 0);
    /* refusals: every one is terminated inside err and names what it refuses */
    refused(N, 1, 1, 0, 0, NULL, 1, 0, NULL, 1, x, out, "K = 0");
    refused(N, 1, 1, 9, 0, NULL, 9, 0, NULL, 1, x, out, "K = 9");
    refused(N, 1, 1, -1, 0, NULL, 1, 0, NULL, 1, x, out, "K = -1");
    refused(N, 1, 1, (int32_t)0x80000000, 0, NULL, 1, 0, NULL, 1, x, out, "K = -2147483648");
    refused(N, 1, LIM + 1, 1, 0, NULL, 1, 0, NULL, 1, x, out, "exactness domain");
    refused(N, 8, LIM / 8 + 1, 8, 0, NULL, 8, 0, NULL, 1, x, out, "exactness domain");
    refused(N, 2, LIM / 2 + 1, 2, 0, NULL, 2, 0, NULL, 1, x, out, "K * wmax = 2 * 98305");
    refused(N, 1, (int64_t)N << 31, 8, 0, NULL, 8, 0, NULL, 1, x, out, "exactness domain");        /* the largest wmax a set can have: no overflow */
    refused(N, 1, -1, 1, 0, NULL, 1, 0, NULL, 1, x, out, "exactness domain");
    refused(N, 0, 1, 1, 0, NULL, 1, 0, NULL, 1, x, out, "n_w = 0");
    refused(N, 1, 1, 1, 0, NULL, 0, 0, NULL, 1, x, out, "n_x = 0");
    refused(N, 1, 1, 1, 0, NULL, -5, 0, NULL, 1, x, out, "n_x = -5");
    refused(N, 1, 1, 1, 0, NULL, 1, 0, NULL, (size_t)1 << 31, x, out, "count * K");
    refused(N, 8, 1, 8, 0, NULL, 8, 0, NULL, ((size_t)1 << 31) / 8, x, out, "count * K");
    refused(N, 1, 1, 1, 0, NULL, 1, 0, NULL, ~(size_t)0, x, out, "count * K");
    refused(N, 2, 1, 3, 0, NULL, 3, 0, NULL, 1, x, out, "w_idx NULL");
    refused(N, 3, 1, 3, 0, NULL, 8, 0, NULL, 3, x, out, "x_idx NULL: sample 2");
    refused(N, 1, 1, 1, 0, NULL, 1, 0, NULL, 1, NULL, out, "null");
    refused(N, 1, 1, 1, 0, NULL, 1, 0, NULL, 1, x, NULL, "null");
    refused(N, 1, 1, 1, 0, NULL, 3, 0, NULL, 3, x, x, "overlaps");
    refused(N, 1, 1, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base + 3 * 2 * N * 4 - 4), "overlaps");
    refused(N, 1, 1, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base - 3 * 2 * N * 4 + 4), "overlaps");
    {   /* one x row read by five samples: out may not touch that one row, wherever the samples' own rows would have been */
        int32_t *xi = indices(5, 1, 0);
        CHECK(plan(N, 1, 1, 1, 0, NULL, 1, 1, xi, 5, x, AT(base + 2 * N * 4)) == 0);
        refused(N, 1, 1, 1, 0, NULL, 1, 1, xi, 5, x, AT(base + 2 * N * 4 - 4), "overlaps");
        free(xi);
    }
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_plain_plan(N, 1, 1, 9, 0, NULL, 1, 0, NULL, 1, x, out, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_plain_plan(N, 1, 1, 9, 0, NULL, 1, 0, NULL, 1, x, out, NULL, 0) == RTFHE_ERR_INVALID);
    }
    {
        const size_t rows[2] = {((size_t)1 << 18) + 3, ((size_t)1 << 20) + 4};
        for (int t = 0; t < 2; t++) {
            large_cases(large_x, rows[t], rows[t] * 16384, 64 * 16384, 4, "overlaps");
            large_cases(large_out, rows[t], 64 * 16384, rows[t] * 16384, 4, "overlaps");
        }
        large_limit(large_out, 0x7fffffff, 0, "count * K");
    }
    printf("plain sanitizer walk ok\n");
    return 0;
}
