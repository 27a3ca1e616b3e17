/* Walks the host-only part of rtfhe_pack_batch[_dev] (rtfhe_pack_plan in rustfhe_amd/csrc/rtfhe_extract_plan.cpp: every argument check that
 * needs no context) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: this code runs before any HIP call.  The position
 * lists are heap arrays of exactly P entries and the shift array is allocated at exactly the size the header promises, so that a read or a
 * write past either is caught; the two buffers are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_extract_plan.h"

/* shift has room for P entries when 1 <= P <= N and for one entry otherwise, as rtfhe_pack.hip sizes it */
static int plan(int32_t N, int32_t P, const int32_t *pos, int32_t rep, size_t count, const void *in, const void *out, int32_t **shift) {
    *shift = malloc(sizeof(int32_t) * (size_t)(P >= 1 && P <= N ? P : 1));
    CHECK(*shift);
    memset(err, 'x', sizeof err);
    return rtfhe_pack_plan(N, P, pos, rep, count, in, out, *shift, err, sizeof err);
}

static void refused(int32_t N, int32_t P, const int32_t *pos, int32_t rep, size_t count, const void *in, const void *out, const char *word) {
    int32_t *shift;
    CHECK(plan(N, P, pos, rep, count, in, out, &shift) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
    free(shift);
}

/* a heap list of exactly P entries: fill everywhere, then `v` at entry `at` */
static int32_t *list(int32_t P, int32_t fill, int32_t at, int32_t v) {
    int32_t *pos = malloc(sizeof(int32_t) * (size_t)P);
    CHECK(pos);
    for (int32_t p = 0; p < P; p++) pos[p] = fill;
    pos[at] = v;
    return pos;
}

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
/* (the packing key switch compares no addresses: the item rule alone) */
static int32_t large_shift[1024];
static int large_plan(size_t count, const void *in, const void *out) {
    memset(err, 'x', sizeof err);
    return rtfhe_pack_plan(1024, 1024, NULL, 1, count, in, out, large_shift, err, sizeof err);
}

int main(void) {
    enum { N = 1024 };
    const void *in = AT(0x10000000), *out = AT(0x40000000);
    int32_t *shift, *pos;
    /* P and rep at 1 and at N; pos NULL: p * rep, up to the last position 2N - 1 */
    CHECK(plan(N, 1, NULL, 1, 1, in, out, &shift) == 0 && err[0] == 0 && shift[0] == 0);
    free(shift);
    CHECK(plan(N, N, NULL, 1, 3, in, out, &shift) == 0 && shift[0] == 0 && shift[N - 1] == N - 1);
    free(shift);
    CHECK(plan(N, 1, NULL, N, 1, in, out, &shift) == 0 && shift[0] == 0);
    free(shift);
    CHECK(plan(N, 2, NULL, N, 1, in, out, &shift) == 0 && shift[1] == N);
    free(shift);
    CHECK(plan(N, N, NULL, 2, 1, in, out, &shift) == 0 && shift[N - 1] == 2 * N - 2);
    free(shift);
    /* a list with duplicates and both ends; rep is then only range-checked */
    pos = list(5, 7, 0, 0);
    pos[4] = 2 * N - 1;
    CHECK(plan(N, 5, pos, N, 2, in, out, &shift) == 0 && err[0] == 0 && !memcmp(shift, pos, 5 * sizeof(int32_t)));
    free(shift);
    free(pos);
    pos = list(N, 2 * N - 1, 0, 0);                                                       /* a whole list of P = N entries */
    CHECK(plan(N, N, pos, 1, 1, in, out, &shift) == 0 && shift[0] == 0 && shift[N - 1] == 2 * N - 1);
    free(shift);
    free(pos);
    CHECK(plan(N, 1, NULL, 1, 0, in, out, &shift) == 0);                                  /* count = 0 */
    free(shift);
    CHECK(plan(N, 1, NULL, 1, 0x7fffffff, in, out, &shift) == 0);                         /* the largest count * P = 2^31 - 1 */
    free(shift);
    CHECK(plan(N, 1, NULL, 1, 3, in, in, &shift) == 0);                                   /* the addresses are not compared */
    free(shift);
    /* refusals: every one is terminated inside err and names what it refuses */
    refused(N, 0, NULL, 1, 1, in, out, "P = 0");
    refused(N, -3, NULL, 1, 1, in, out, "P = -3");
    refused(N, N + 1, NULL, 1, 1, in, out, "P = 1025");
    refused(N, 0x7fffffff, NULL, 1, 1, in, out, "P = 2147483647");
    refused(N, 1, NULL, 0, 1, in, out, "rep = 0");
    refused(N, 1, NULL, N + 1, 1, in, out, "rep = 1025");
    refused(N, 1, NULL, (int32_t)0x80000000, 1, in, out, "rep = -2147483648");
    pos = list(3, 5, 1, -1);
    refused(N, 3, pos, 1, 1, in, out, "sample 1: pos = -1 is outside [0, 2048)");
    pos[1] = 2 * N;
    refused(N, 3, pos, 1, 1, in, out, "sample 1: pos = 2048");
    pos[1] = (int32_t)0x80000000;
    refused(N, 3, pos, 1, 1, in, out, "sample 1: pos = -2147483648");
    free(pos);
    refused(16, 3, NULL, 16, 1, in, out, "sample 2: pos = 32 is outside [0, 32) (pos NULL: p * rep)");      /* N = 16: p * rep trips at p = 2 */
    refused(N, 1, NULL, 1, (size_t)1 << 31, in, out, "count * P");
    refused(N, 5, NULL, 1, ((size_t)1 << 31) / 5 + 1, in, out, "count * P");
    refused(N, 1, NULL, 1, ~(size_t)0, in, out, "count * P");
    refused(N, 1, NULL, 1, 1, NULL, out, "null");
    refused(N, 1, NULL, 1, 1, in, NULL, "null");
    CHECK(rtfhe_pack_plan(N, 1, NULL, 1, 1, in, out, NULL, err, sizeof err) == RTFHE_ERR_INVALID);      /* no room for the positions */
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        pos = list(1, -1, 0, -1);
        shift = malloc(sizeof(int32_t));
        CHECK(shift && rtfhe_pack_plan(N, 1, pos, 1, 1, in, out, shift, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_pack_plan(N, 1, pos, 1, 1, in, out, shift, NULL, 0) == RTFHE_ERR_INVALID);
        free(shift);
        free(pos);
    }
    large_limit(large_plan, (size_t)0x7fffffff / 1024, 1024 * 4 * 9, "count * P");
    printf("pack sanitizer walk ok\n");
    return 0;
}
