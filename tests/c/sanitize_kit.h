/* What every *_sanitize_main.c of this directory opens with: the C headers, CHECK, the message buffer a walk poisons before each call (so that a
 * missing terminator shows) and AT(), an address that is never dereferenced. */
#ifndef SANITIZE_KIT_H
#define SANITIZE_KIT_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static char err[200] __attribute__((unused));

/* addresses only: integers, so that no pointer arithmetic leaves an object */
#define AT(a) ((const void *)(uintptr_t)(a))

/* Buffers past 4 GiB and 16 GiB ("Address arithmetic"; the same cases as tests/test_large_plans_host.py, here so that
 * UndefinedBehaviorSanitizer sees the arithmetic).  plan(items, in, out): the walk's own call of its plan function with everything else fixed,
 * its message left in err.  For `items` items whose input is in_bytes and whose output is out_bytes, at least one of them above 2^32: an output
 * directly behind and directly before the input is accepted; one that shares only the input's last `last` bytes, or whose last `last` bytes are
 * the input's first, is refused with `word` in the message, and so is one that starts half a row inside the far end of the larger buffer; starts
 * exactly 2^32 and 2^33 bytes apart overlap only where a buffer reaches that far.  Then the item rule: `limit` items pass, limit + 1, 2^32 and
 * 2^32 + 1 are refused with `rule` in the message (limit = 0: the family's rule is not about these items). */
typedef int (*large_plan_fn)(size_t items, const void *in, const void *out);
#define LARGE_BASE ((uintptr_t)0x7F0000000000ull)      /* 127 TiB: every case stays far below 2^63 */
#define LARGE_FAR ((uintptr_t)0x100000000000ull)       /* 16 TiB */

static void large_cases(large_plan_fn plan, size_t items, size_t in_bytes, size_t out_bytes, size_t last, const char *word) __attribute__((unused));
static void large_cases(large_plan_fn plan, size_t items, size_t in_bytes, size_t out_bytes, size_t last, const char *word) {
    const uintptr_t a = LARGE_BASE;
    const int far_out = out_bytes > in_bytes;
    const size_t half = (far_out ? out_bytes : in_bytes) / items / 2 / 16 * 16;
    const uintptr_t refused[3] = {a + in_bytes - last, a - out_bytes + last, far_out ? a - out_bytes + half : a + in_bytes - half};
    CHECK(in_bytes > ((size_t)1 << 32) || out_bytes > ((size_t)1 << 32));
    CHECK(plan(items, AT(a), AT(a + in_bytes)) == 0 && err[0] == 0);
    CHECK(plan(items, AT(a), AT(a - out_bytes)) == 0 && err[0] == 0);
    for (int k = 0; k < 3; k++) {
        memset(err, 'x', sizeof err);
        CHECK(plan(items, AT(a), AT(refused[k])) == RTFHE_ERR_INVALID && memchr(err, 0, sizeof err) && strstr(err, word));
    }
    for (int k = 32; k <= 33; k++) {
        const size_t d = (size_t)1 << k;
        CHECK((plan(items, AT(a), AT(a + d)) != 0) == (d < in_bytes));
        CHECK((plan(items, AT(a), AT(a - d)) != 0) == (d < out_bytes));
    }
}

static void large_limit(large_plan_fn plan, size_t limit, size_t in_bytes_per_item, const char *rule) __attribute__((unused));
static void large_limit(large_plan_fn plan, size_t limit, size_t in_bytes_per_item, const char *rule) {
    const size_t over[3] = {limit + 1, (size_t)1 << 32, ((size_t)1 << 32) + 1};
    CHECK(plan(limit, AT(LARGE_BASE), AT(LARGE_BASE + limit * in_bytes_per_item + LARGE_FAR)) == 0 && err[0] == 0);
    for (int k = 0; k < 3; k++) {
        memset(err, 'x', sizeof err);
        CHECK(plan(over[k], AT(LARGE_BASE), AT(LARGE_BASE + over[k] * in_bytes_per_item + LARGE_FAR)) == RTFHE_ERR_INVALID && strstr(err, rule));
    }
}

#endif
