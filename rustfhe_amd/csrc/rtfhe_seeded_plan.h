/* rtfhe_seeded_plan.h -- the host-only argument checks of the seeded-ciphertext calls (include/rtfhe.h: rtfhe_mask_expand, rtfhe_seeded_expand[_dev]
 * and the *_seeded upload calls of ring rows; rtfhe_tlwe_seeded_expand[_dev] and rtfhe_load_ksk_seeded of lvl0 rows), with no device call in them
 * (rtfhe_seeded.cpp).  Internal: rtfhe_seeded.hip, rtfhe_context.hip and the upload calls run them before anything is allocated or launched, and
 * tests/c/seeded_sanitize_main.c and tests/c/tlwe_seeded_sanitize_main.c walk them under the host sanitizers.  Plain C so that a C host can
 * include it. */
#ifndef RTFHE_SEEDED_PLAN_H
#define RTFHE_SEEDED_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ring rows (length N) ---- */
/* what is being checked: the CPU expansion, the device expansion (also: 16-byte aligned pointers, rows * N / 16 below 2^31 lanes), or an upload
 * call, whose output is the library's own buffer (out is not looked at) */
#define RTFHE_SEEDED_HOST 0
#define RTFHE_SEEDED_DEVICE 1
#define RTFHE_SEEDED_UPLOAD 2

/* The checks of one call, in this order: seed, b and (unless an upload) out non-null; N a power of two in 16 .. 2048; group >= 1; rows a multiple of
 * group; first_row + rows <= 2^64; the device forms' alignment and size; b [rows][N] overlaps no part of out [2 rows][N] (u32 words; compared as
 * addresses and never dereferenced).  Returns 0, or RTFHE_ERR_INVALID with a message in err (always terminated; err_len >= 1). */
int rtfhe_seeded_plan(int32_t what, int32_t N, const void *seed, uint64_t first_row, const void *b, int32_t group, const void *out, size_t rows,
                      char *err, size_t err_len);

/* ---- lvl0 rows (length n) ---- */
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
