// rtfhe_plain_plan.cpp -- host only: the argument checks of the TRLWE x plain-polynomial product (rtfhe_plain_plan.h), before rtfhe_plain_create
// and rtfhe_trlwe_mul_plain_batch[_dev] (rtfhe_plain.hip) allocate or launch anything.  Written with rtfhe_plan_kit.hpp; the call's checks are
// the kit's sum-of-products body, which rtfhe_trgsw_mac_plan shares, with the exactness domain in front.
#include "rtfhe_plain_plan.h"

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

extern "C" int rtfhe_plain_weights_plan(int32_t N, const int32_t* w, int32_t n_w, int64_t* wmax, char* err, size_t err_len) {
    begin(err, err_len);
    if (!w || !wmax) return refuse(err, err_len, "null argument");
    *wmax = 0;
    if (N < 1) return refuse(err, err_len, "N = " + num(N) + " is below 1");
    if (n_w < 1) return refuse(err, err_len, "n_w = " + num(n_w) + " is below 1");
    if (!count_fits((size_t)n_w, (size_t)N)) return refuse(err, err_len, "n_w * N too large (it must be below 2^31)");
    for (int32_t e = 0; e < n_w; e++) {
        int64_t l1 = 0;
        for (int32_t c = 0; c < N; c++) {
            const int64_t v = w[(size_t)e * N + c];
            l1 += v < 0 ? -v : v;
        }
        if (l1 > *wmax) *wmax = l1;
    }
    return 0;
}

extern "C" int rtfhe_plain_plan(int32_t N, int32_t n_w, int64_t wmax, int32_t K, int32_t w_idx_given, const int32_t* w_idx, int32_t n_x,
                                int32_t x_idx_given, const int32_t* x_idx, size_t count, const void* x, const void* out, char* err, size_t err_len) {
    if (int rc = terms_head(N, K, RTFHE_PLAIN_K_MAX, x, out, err, err_len)) return rc;
    const int64_t limit = (int64_t)RTFHE_PLAIN_L1_PER_N * N;
    if (wmax < 0 || wmax > limit / K)      // K * wmax <= limit, without the product (wmax goes up to N * 2^31)
        return refuse(err, err_len, "K * wmax = " + num(K) + " * " + num(wmax) + " is above the exactness domain " + num(RTFHE_PLAIN_L1_PER_N) + " * N = " + num(limit));
    return terms_tail(N, K, "n_w", TermIdx{"w_idx", "weights", "the set", n_w, w_idx_given != 0, w_idx, true},
                      TermIdx{"x_idx", "rows", "x", n_x, x_idx_given != 0, x_idx, false}, count, x, out, err, err_len);
}
