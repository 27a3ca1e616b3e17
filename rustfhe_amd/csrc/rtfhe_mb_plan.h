/* rtfhe_mb_plan.h -- the host-only part of the multi-bit blind rotation (include/rtfhe.h: rtfhe_mbk_*, rtfhe_pbs_mb_batch[_dev]): the sizes of a
 * multi-bit key, the roots table and the point map behind the frequency-domain key combination (both public, declared in include/rtfhe.h), and
 * every argument check that needs no context, with no device call in it (rtfhe_mb_plan.cpp).  Internal: rtfhe_pbs_mb.hip calls the checks before
 * anything is allocated or launched, and tests/c/mb_sanitize_main.c walks them under the host sanitizers.  Plain C so that a C host can include it. */
#ifndef RTFHE_MB_PLAN_H
#define RTFHE_MB_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* key bits per step: g = 2 or 3 */
#define RTFHE_MB_G_MIN 2
#define RTFHE_MB_G_MAX 3

/* Group t of a key of n bits covers bits [t g, min(n, t g + g)): ceil(n / g) groups, the last one ragged when g does not divide n.  A group of
 * g' bits holds 2^g' - 1 TRGSW samples, subsets j = 1 .. 2^g' - 1 in order.  Both return -1 for n < 1 or g outside [2, 3].  Inline: the key
 * generator (rtfhe_keygen.cpp), a host-only unit that is also built on its own, counts with them too. */
static inline int64_t rtfhe_mb_group_count(int32_t n, int32_t g) {
    return n < 1 || g < RTFHE_MB_G_MIN || g > RTFHE_MB_G_MAX ? -1 : ((int64_t)n + g - 1) / g;
}
static inline int64_t rtfhe_mb_trgsw_count(int32_t n, int32_t g) {
    return n < 1 || g < RTFHE_MB_G_MIN || g > RTFHE_MB_G_MAX ? -1 : (int64_t)(n / g) * (((int64_t)1 << g) - 1) + (((int64_t)1 << (n % g)) - 1);
}

/* The checks of a key upload, in this order: words non-null; g in [2, 3]; n >= 1; N 1024 or 2048; l >= 1; the TRGSW count times the 4 l
 * polynomials of one stays below 2^31.  Returns 0, or RTFHE_ERR_INVALID with a message in err (always terminated; err_len >= 1). */
int rtfhe_mb_key_plan(int32_t n, int32_t N, int32_t l, int32_t g, const void *words, char *err, size_t err_len);

/* The checks of one call, in this order: tlwe and out non-null; g in [2, 3]; n >= 1; count below 2^31; n_lut >= 1; every entry of the host
 * array lut_idx (null in the _dev form, whose array the kernel checks, and where the caller passed none) in [0, n_lut), the first offender
 * named.  The buffers are addresses only and are never dereferenced.  count == 0 passes.
 * Returns 0, or RTFHE_ERR_INVALID with a message in err (always terminated; err_len >= 1). */
int rtfhe_mb_call_plan(int32_t n, int32_t g, size_t count, const int32_t *lut_idx, int32_t n_lut, const void *tlwe, const void *out, char *err,
                       size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
