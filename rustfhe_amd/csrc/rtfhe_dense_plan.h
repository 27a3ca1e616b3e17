/* rtfhe_dense_plan.h -- the host-only part of rtfhe_dense_create and rtfhe_tlwe_dense_batch[_dev] (include/rtfhe.h): every argument check that
 * needs no context, the per-output correction words and the launch rule, with no device call in it (rtfhe_dense_plan.cpp).  Internal:
 * rtfhe_dense.hip calls it before anything is allocated or launched, and tests/c/dense_sanitize_main.c walks it under the host sanitizers.
 * Plain C so that a C host can include it. */
#ifndef RTFHE_DENSE_PLAN_H
#define RTFHE_DENSE_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most outputs and inputs of a layer, and the outputs one launch carries bias words for in its arguments (a call with a bias is one launch
 * per RTFHE_DENSE_BIAS_PER_LAUNCH outputs, as rtfhe_trlwe_extract_batch_dev is one per 512 coefficients) */
#define RTFHE_DENSE_MAX 65536
#define RTFHE_DENSE_BIAS_PER_LAUNCH 512

/* The checks of a matrix, in this order: W and corr non-null; 1 <= O, I <= RTFHE_DENSE_MAX (before W is read); every entry in [-128, 127], the
 * first offender named by row and column.  corr[o] = 128 * 0x01010101 * sum_i W[o][i] mod 2^32: what the kernel's signed byte limbs
 * (u - 128 per byte of a ciphertext word) drop from every word of output o.
 * Returns 0, or RTFHE_ERR_INVALID with a message in err (always terminated; err_len >= 1); corr is written only on success. */
int rtfhe_dense_weights_plan(const int32_t *W, int32_t O, int32_t I, uint32_t *corr /* [O] */, char *err, size_t err_len);

/* The checks of one call, in this order: x and out non-null; 1 <= n; 1 <= O, I <= RTFHE_DENSE_MAX; count * max(I, O) * (n + 1) < 2^31 words;
 * out [count][O][n+1] overlaps no part of x [count][I][n+1] (u32 words; compared as addresses and never dereferenced).  count == 0 passes.
 * Returns 0, or RTFHE_ERR_INVALID with a message in err (always terminated; err_len >= 1). */
int rtfhe_dense_plan(int32_t n, int32_t O, int32_t I, size_t count, const void *x, const void *out, char *err, size_t err_len);

/* THE launch rule.  A wave owns RTFHE_DENSE_CT = 2 tiles of 16 words and `tiles` = 1, 2 or 4 tiles of 16 outputs (the most that O fills), a
 * workgroup four waves on neighbouring words.  When the workgroups of a call (count * output groups * ceil(ceil((n+1)/32) / 4)) number fewer
 * than two per CU and I has K-steps (of 64 inputs) to share out, I is cut into `slices` runs of `steps` K-steps, at least two each, whose parts
 * meet in the output as wrapping u32 atomics; slices == 1 means plain stores.  Arguments must have passed rtfhe_dense_plan; cus >= 1. */
#define RTFHE_DENSE_CT 2
typedef struct rtfhe_dense_shape { int32_t tiles, groups, cwgs, ksteps, slices, steps; } rtfhe_dense_shape;
void rtfhe_dense_launch_shape(int32_t n, int32_t O, int32_t I, size_t count, int32_t cus, rtfhe_dense_shape *shape);

#ifdef __cplusplus
}
#endif

#endif
