/* rtfhe_tlwe_seeded_plan.h -- the host-only argument checks of the seeded lvl0 calls (include/rtfhe.h: rtfhe_tlwe_seeded_expand[_dev] and
 * rtfhe_load_ksk_seeded), with no device call in it (rtfhe_tlwe_seeded.cpp).  Internal: rtfhe_seeded.hip and rtfhe_context.hip run it before
 * anything is allocated or launched, and tests/c/tlwe_seeded_sanitize_main.c walks it under the host sanitizers.  Plain C so that a C host can
 * include it. */
#ifndef RTFHE_TLWE_SEEDED_PLAN_H
#define RTFHE_TLWE_SEEDED_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* what is being checked: the CPU expansion (any n >= 1), the device expansion of a context (also: n <= 767, rows * ceil(n / 16) below 2^31 lanes,
 * 4-byte aligned pointers), or an upload call of a context, whose output is the library's own buffer (out is not looked at) */
#define RTFHE_TLWE_SEEDED_HOST 0
#define RTFHE_TLWE_SEEDED_DEVICE 1
#define RTFHE_TLWE_SEEDED_UPLOAD 2

/* The checks of one call, in this order: seed, b and (unless an upload) out non-null; n >= 1 (a context's calls: n <= 767); rows >= 1;
 * first_row + rows <= 2^64; the size (a context's calls: rows * ceil(n / 16) below 2^31; the CPU form: rows * (n + 1) words addressable); the
 * device form's alignment; b [rows] overlaps no part of out [rows][n + 1] (u32 words; compared as addresses and never dereferenced).  Returns 0, or
 * RTFHE_ERR_INVALID with a message in err (always terminated; err_len >= 1). */
int rtfhe_tlwe_seeded_plan(int32_t what, int32_t n, const void *seed, uint64_t first_row, const void *b, const void *out, size_t rows, char *err,
                           size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
