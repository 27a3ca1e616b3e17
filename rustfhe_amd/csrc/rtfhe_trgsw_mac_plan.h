/* rtfhe_trgsw_mac_plan.h -- the host-only part of rtfhe_trlwe_mul_trgsw_batch[_dev] (include/rtfhe.h): every argument check that needs no
 * context, with no device call in it (rtfhe_trgsw_mac_plan.cpp).  Internal: rtfhe_trgsw_mac.hip calls it before anything is allocated or
 * launched, and tests/c/trgsw_mac_sanitize_main.c walks it under the host sanitizers.  Plain C so that a C host can include it. */
#ifndef RTFHE_TRGSW_MAC_PLAN_H
#define RTFHE_TRGSW_MAC_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most terms of one sum: K * 2l * N * (Bg/2) * 2^31 stays below 2^53 at N = 2048 */
#define RTFHE_TRGSW_MAC_K_MAX 8

/* The checks of one call, in this order: x and out non-null; 1 <= K <= RTFHE_TRGSW_MAC_K_MAX; n_sel, n_x >= 1; count * K < 2^31;
 * s_idx not given: n_sel >= count * K; x_idx not given: n_x >= count * K; every entry of a host index array in range;
 * out [count][2][N] overlaps no part of x [n_x][2][N] (u32 words; compared as addresses and never dereferenced).
 * s_idx_given / x_idx_given say whether the caller passed an index array; s_idx / x_idx are the HOST arrays [count][K] to walk, null when the
 * array lives on the device (the kernel then checks it) or was not given.
 * Returns 0, or RTFHE_ERR_INVALID with a message naming the sample in err (always terminated; err_len >= 1). */
int rtfhe_trgsw_mac_plan(int32_t N, int32_t n_sel, int32_t K, int32_t s_idx_given, const int32_t *s_idx, int32_t n_x, int32_t x_idx_given,
                         const int32_t *x_idx, size_t count, const void *x, const void *out, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
