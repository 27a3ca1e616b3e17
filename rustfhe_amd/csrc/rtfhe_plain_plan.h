/* rtfhe_plain_plan.h -- the host-only part of rtfhe_plain_create and rtfhe_trlwe_mul_plain_batch[_dev] (include/rtfhe.h): every argument check
 * that needs no context, with no device call in it (rtfhe_plain_plan.cpp).  Internal: rtfhe_plain.hip calls it before anything is allocated or
 * launched, and tests/c/plain_sanitize_main.c walks it under the host sanitizers.  Plain C so that a C host can include it. */
#ifndef RTFHE_PLAIN_PLAN_H
#define RTFHE_PLAIN_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most terms of one product, and the exactness domain's factor: a call is accepted iff K * wmax <= RTFHE_PLAIN_L1_PER_N * N, the total l1
 * norm 6 * 32 * N the split-FFT exact backend is proven at (scripts/xfft/model.py: error_bound) */
#define RTFHE_PLAIN_K_MAX 8
#define RTFHE_PLAIN_L1_PER_N 192

/* wmax = max over the n_w polynomials w[e], int32[N], of their l1 norm (sum of |coefficient|; at most N * 2^31, exact in int64).
 * Returns 0, or RTFHE_ERR_INVALID (w or wmax null, n_w < 1, n_w * N >= 2^31) with a message in err (always terminated; err_len >= 1). */
int rtfhe_plain_weights_plan(int32_t N, const int32_t *w, int32_t n_w, int64_t *wmax, char *err, size_t err_len);

/* The checks of one product call, in this order: x and out non-null; 1 <= K <= RTFHE_PLAIN_K_MAX; K * wmax <= RTFHE_PLAIN_L1_PER_N * N;
 * n_w, n_x >= 1; count * K < 2^31; w_idx not given: n_w >= K; x_idx not given: n_x >= count * K; every entry of a host index array in range;
 * out [count][2][N] overlaps no part of x [n_x][2][N] (u32 words; compared as addresses and never dereferenced).
 * w_idx_given / x_idx_given say whether the caller passed an index array; w_idx / x_idx are the HOST arrays [count][K] to walk, null when the
 * array lives on the device (the kernel then checks it) or was not given.
 * Returns 0, or RTFHE_ERR_INVALID with a message naming the sample in err (always terminated; err_len >= 1). */
int rtfhe_plain_plan(int32_t N, int32_t n_w, int64_t wmax, int32_t K, int32_t w_idx_given, const int32_t *w_idx, int32_t n_x, int32_t x_idx_given,
                     const int32_t *x_idx, size_t count, const void *x, const void *out, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
