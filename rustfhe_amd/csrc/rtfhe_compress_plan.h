/* rtfhe_compress_plan.h -- the host-only part of compressed results (include/rtfhe.h: rtfhe_tlwe_compress_batch_dev,
 * rtfhe_trlwe_compress_batch_dev, rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev and the CPU twins rtfhe_tlwe_compress / _expand,
 * rtfhe_trlwe_compress / _expand): every argument check, the row size, the coefficient list, its inverse map and the CPU forms, with no device
 * call in them (rtfhe_compress_plan.cpp).  Internal: rtfhe_compress.hip runs the checks before anything is launched, and
 * tests/c/compress_sanitize_main.c and tests/c/expand_sanitize_main.c walk them and the twins under the host sanitizers.  Plain C so that a C
 * host can include it. */
#ifndef RTFHE_COMPRESS_PLAN_H
#define RTFHE_COMPRESS_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* which side of a call is full rows and which is packed words: a compression (in: full rows, out: [count][W]) or an expansion (the reverse) */
#define RTFHE_COMPRESS_PACK 0
#define RTFHE_COMPRESS_EXPAND 1

/* The checks of one lvl0 call, in this order: in and out non-null; n >= 1; k in 2 .. 32; count * (n + 1) < 2^31; the full rows [count][n + 1] and
 * the packed rows [count][W(n + 1, k)] do not overlap (u32 words; compared as addresses and never dereferenced).  Returns 0, or RTFHE_ERR_INVALID
 * with a message in err (always terminated; err_len >= 1; err may be NULL). */
int rtfhe_tlwe_compress_plan(int32_t dir, int32_t n, int32_t k, size_t count, const void *in, const void *out, char *err, size_t err_len);

/* The checks of one TRLWE call: in, out and idx non-null; k in 2 .. 32; the coefficient list by rtfhe_extract_plan's rules (1 <= P <= N; coef[p] in
 * [0, N), coef NULL: p * stride with stride >= 1) and its message; count * (N + P) < 2^31; the full rows [count][2][N] and the packed rows
 * [count][W(N + P, k)] do not overlap.  On success idx[0 .. P) holds the coefficients (idx has room for P entries whenever 1 <= P <= N). */
int rtfhe_trlwe_compress_plan(int32_t dir, int32_t N, int32_t k, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *in,
                              const void *out, int32_t *idx, char *err, size_t err_len);

/* The expansion's view of a coefficient list (rtfhe_trlwe_expand_batch_dev): inv[j] = the LAST p in [0, P) with idx[p] == j, or -1 where no
 * entry names j, for j in [0, N) -- "the later entry wins", decided here once and not by racing stores on the device.  idx is what
 * rtfhe_trlwe_compress_plan resolved.  int16 holds every p: returns RTFHE_ERR_INVALID, with inv untouched, for a null pointer, N outside
 * 1 .. 32768, P outside 1 .. N or an idx[p] outside [0, N); else 0. */
int rtfhe_expand_inverse_map(int32_t N, int32_t P, const int32_t *idx, int16_t *inv /* [N] */);

#ifdef __cplusplus
}
#endif

#endif
