/* rtfhe_extract_plan.h -- the host-only part of rtfhe_trlwe_extract_batch[_dev] and rtfhe_trlwe_extract_lvl1_batch[_dev] and of their inverse,
 * rtfhe_pack_batch[_dev] (include/rtfhe.h): every argument check that needs no context, with no device call in it (rtfhe_extract_plan.cpp).
 * Internal: rtfhe_extract.hip and rtfhe_pack.hip call it before anything is allocated or launched, and tests/c/extract_sanitize_main.c and
 * pack_sanitize_main.c walk it under the host sanitizers.  Plain C so that a C host can include it. */
#ifndef RTFHE_EXTRACT_PLAN_H
#define RTFHE_EXTRACT_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Checks 1 <= P <= N, count * P < 2^31, every coef[p] in [0, N) -- with coef NULL stride >= 1 and the coefficients p * stride it stands for,
 * i.e. (P - 1) * stride < N -- and that out [count * P][out_words] does not overlap in [count][2][N] (u32 words; both non-null; they are
 * compared as addresses and never dereferenced).  On success idx[0 .. P) holds the coefficients (idx has room for P entries whenever 1 <= P <= N).
 * Returns 0, or RTFHE_ERR_INVALID with a message naming the sample in err (always terminated; err_len >= 1). */
int rtfhe_extract_plan(int32_t N, int32_t P, const int32_t *coef, int32_t stride, size_t count, const void *in, const void *out,
                       size_t out_words, int32_t *idx, char *err, size_t err_len);

/* The inverse, the packing key switch (rtfhe_pack_batch[_dev], rtfhe_pack.hip; walked by tests/c/pack_sanitize_main.c): checks 1 <= P <= N,
 * 1 <= rep <= N, count * P < 2^31 and every pos[p] in [0, 2N) -- with pos NULL the positions p * rep it stands for.  in and out are non-null and
 * otherwise not looked at.  On success shift[0 .. P) holds the positions (shift has room for P entries whenever 1 <= P <= N).  Returns 0, or
 * RTFHE_ERR_INVALID with a message naming the sample in err (always terminated; err_len >= 1). */
int rtfhe_pack_plan(int32_t N, int32_t P, const int32_t *pos, int32_t rep, size_t count, const void *in, const void *out, int32_t *shift, char *err,
                    size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
