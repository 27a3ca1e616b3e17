// rtfhe_trgsw_mac_plan.cpp -- host only: the argument checks of the TRLWE x TRGSW multiply-accumulate (rtfhe_trgsw_mac_plan.h), before
// rtfhe_trlwe_mul_trgsw_batch[_dev] (rtfhe_trgsw_mac.hip) allocates or launches anything: the sum-of-products body of rtfhe_plan_kit.hpp, which
// rtfhe_plain_plan shares.
#include "rtfhe_trgsw_mac_plan.h"

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

extern "C" int rtfhe_trgsw_mac_plan(int32_t N, int32_t n_sel, int32_t K, int32_t s_idx_given, const int32_t* s_idx, int32_t n_x, int32_t x_idx_given,
                                    const int32_t* x_idx, size_t count, const void* x, const void* out, char* err, size_t err_len) {
    if (int rc = terms_head(N, K, RTFHE_TRGSW_MAC_K_MAX, x, out, err, err_len)) return rc;
    return terms_tail(N, K, "n_sel", TermIdx{"s_idx", "selectors", "the set", n_sel, s_idx_given != 0, s_idx, false},
                      TermIdx{"x_idx", "rows", "x", n_x, x_idx_given != 0, x_idx, false}, count, x, out, err, err_len);
}
