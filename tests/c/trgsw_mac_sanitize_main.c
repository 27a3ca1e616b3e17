/* Walks the host-only part of rtfhe_trlwe_mul_trgsw_batch[_dev] (rustfhe_amd/csrc/rtfhe_trgsw_mac_plan.cpp: every argument check that needs no
 * context) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this code runs before any HIP call.  The index arrays are
 * allocated at exactly the sizes the header promises, so that a read past them is caught; the two buffers are addresses only and are never
 * dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_trgsw_mac_plan.h"

static int plan(int32_t N, int32_t n_sel, int32_t K, int32_t sg, const int32_t *s_idx, int32_t n_x, int32_t xg, const int32_t *x_idx, size_t count,
                const void *x, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_trgsw_mac_plan(N, n_sel, K, sg, s_idx, n_x, xg, x_idx, count, x, out, err, sizeof err);
}

static void refused(int32_t N, int32_t n_sel, int32_t K, int32_t sg, const int32_t *s_idx, int32_t n_x, int32_t xg, const int32_t *x_idx, size_t count,
                    const void *x, const void *out, const char *word) {
    CHECK(plan(N, n_sel, K, sg, s_idx, n_x, xg, x_idx, count, x, out) == RTFHE_ERR_INVALID);
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
static int large_x(size_t rows, const void *x, const void *out) { return plan(2048, 1, 1, 1, NULL, (int32_t)rows, 1, NULL, 64, x, out); }
static int large_out(size_t count, const void *x, const void *out) { return plan(2048, 1, 1, 1, NULL, 64, 1, NULL, count, x, out); }

int main(void) {
    enum { N = 1024 };
    const uintptr_t base = 0x10000000;                                              /* addresses only: integers, so that no pointer arithmetic leaves an object */
    const void *x = AT(base), *out = AT(0x40000000);                                /* far apart: a row is 8 KiB */

    /* accepted: K at both ends; NULL indices at their exact needs; count = 0; the largest count * K */
    CHECK(plan(N, 3, 1, 0, NULL, 3, 0, NULL, 3, x, out) == 0 && err[0] == 0);
    CHECK(plan(N, 24, 8, 0, NULL, 24, 0, NULL, 3, x, out) == 0);
    CHECK(plan(2048, 8, 8, 0, NULL, 8, 0, NULL, 1, x, out) == 0);
    CHECK(plan(N, 1, 1, 0, NULL, 1, 0, NULL, 0, x, out) == 0);
    CHECK(plan(N, 1, 2, 0, NULL, 1, 0, NULL, 0, x, out) == 0);                                      /* count = 0: the NULL-index rules ask for nothing */
    CHECK(plan(N, 1, 1, 1, NULL, 1, 1, NULL, 0x7fffffff, x, AT(0x7000000000000000ull)) == 0);      /* index arrays on the device: not walked */
    CHECK(plan(N, 1, 8, 1, NULL, 1, 1, NULL, 0x7fffffff / 8, x, AT(0x7000000000000000ull)) == 0);
    /* one index array given, the other NULL at its exact need */
    {
        int32_t *si = indices(3, 2, 0);
        CHECK(plan(N, 1, 2, 1, si, 6, 0, NULL, 3, x, out) == 0);
        refused(N, 1, 2, 1, si, 5, 0, NULL, 3, x, out, "x_idx NULL: sample 2 reads rows up to 5, x has 5");
        CHECK(plan(N, 6, 2, 0, NULL, 1, 1, si, 3, x, out) == 0);
        refused(N, 5, 2, 0, NULL, 1, 1, si, 3, x, out, "s_idx NULL: sample 2 reads selectors up to 5, the set has 5");
        free(si);
    }
    {   /* host indices with duplicates and both ends; one selector and one x row shared by all samples */
        int32_t *si = indices(5, 3, 0), *xi = indices(5, 3, 0);
        si[4] = 6; si[14] = 6; xi[7] = 1; xi[14] = 1;
        CHECK(plan(N, 7, 3, 1, si, 2, 1, xi, 5, x, out) == 0);
        si[14] = 7;
        refused(N, 7, 3, 1, si, 2, 1, xi, 5, x, out, "sample 4: s_idx[2] = 7");
        si[14] = -1;
        refused(N, 7, 3, 1, si, 2, 1, xi, 5, x, out, "sample 4: s_idx[2] = -1");
        si[14] = 0; xi[3] = 2;
        refused(N, 7, 3, 1, si, 2, 1, xi, 5, x, out, "sample 1: x_idx[0] = 2");
        xi[3] = (int32_t)0x80000000;
        refused(N, 7, 3, 1, si, 2, 1, xi, 5, x, out, "sample 1: x_idx[0] = -2147483648");
        free(si); free(xi);
    }
    /* out right behind the rows, and right before them, does not overlap */
    CHECK(plan(N, 3, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base + 3 * 2 * N * 4)) == 0);
    CHECK(plan(N, 3, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base - 3 * 2 * N * 4)) == 0);
    /* refusals: every one is terminated inside err and names what it refuses */
    refused(N, 1, 0, 0, NULL, 1, 0, NULL, 1, x, out, "K = 0");
    refused(N, 9, 9, 0, NULL, 9, 0, NULL, 1, x, out, "K = 9");
    refused(N, 1, -1, 0, NULL, 1, 0, NULL, 1, x, out, "K = -1");
    refused(N, 1, (int32_t)0x80000000, 0, NULL, 1, 0, NULL, 1, x, out, "K = -2147483648");
    refused(N, 0, 1, 0, NULL, 1, 0, NULL, 1, x, out, "n_sel = 0");
    refused(N, 1, 1, 0, NULL, 0, 0, NULL, 1, x, out, "n_x = 0");
    refused(N, 1, 1, 0, NULL, -5, 0, NULL, 1, x, out, "n_x = -5");
    refused(0, 1, 1, 0, NULL, 1, 0, NULL, 1, x, out, "N = 0");
    refused(N, 1, 1, 1, NULL, 1, 1, NULL, (size_t)1 << 31, x, out, "count * K");
    refused(N, 8, 8, 1, NULL, 8, 1, NULL, ((size_t)1 << 31) / 8, x, out, "count * K");
    refused(N, 1, 1, 1, NULL, 1, 1, NULL, ~(size_t)0, x, out, "count * K");
    refused(N, 2, 3, 0, NULL, 3, 0, NULL, 1, x, out, "s_idx NULL: sample 0");
    refused(N, 9, 3, 0, NULL, 8, 0, NULL, 3, x, out, "x_idx NULL: sample 2");
    refused(N, 0x7fffffff, 1, 0, NULL, 0x7ffffffe, 0, NULL, 0x7fffffff, x, AT(0x7000000000000000ull), "x_idx NULL");
    refused(N, 1, 1, 0, NULL, 1, 0, NULL, 1, NULL, out, "null");
    refused(N, 1, 1, 0, NULL, 1, 0, NULL, 1, x, NULL, "null");
    refused(N, 3, 1, 0, NULL, 3, 0, NULL, 3, x, x, "overlaps");
    refused(N, 3, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base + 3 * 2 * N * 4 - 4), "overlaps");
    refused(N, 3, 1, 0, NULL, 3, 0, NULL, 3, x, AT(base - 3 * 2 * N * 4 + 4), "overlaps");
    {   /* one x row read by five samples: out may not touch that one row, wherever the samples' own rows would have been */
        int32_t *xi = indices(5, 1, 0);
        CHECK(plan(N, 5, 1, 0, NULL, 1, 1, xi, 5, x, AT(base + 2 * N * 4)) == 0);
        refused(N, 5, 1, 0, NULL, 1, 1, xi, 5, x, AT(base + 2 * N * 4 - 4), "overlaps");
        free(xi);
    }
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_trgsw_mac_plan(N, 1, 9, 0, NULL, 1, 0, NULL, 1, x, out, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_trgsw_mac_plan(N, 1, 9, 0, NULL, 1, 0, NULL, 1, x, out, NULL, 0) == RTFHE_ERR_INVALID);
    }
    {
        const size_t rows[2] = {((size_t)1 << 18) + 3, ((size_t)1 << 20) + 4};
        for (int t = 0; t < 2; t++) {
            large_cases(large_x, rows[t], rows[t] * 16384, 64 * 16384, 4, "overlaps");
            large_cases(large_out, rows[t], 64 * 16384, rows[t] * 16384, 4, "overlaps");
        }
        large_limit(large_out, 0x7fffffff, 0, "count * K");
    }
    printf("trgsw mac sanitizer walk ok\n");
    return 0;
}
