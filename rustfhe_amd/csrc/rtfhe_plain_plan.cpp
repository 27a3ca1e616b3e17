// rtfhe_plain_plan.cpp -- host only: the argument checks of the TRLWE x plain-polynomial product (rtfhe_plain_plan.h), before rtfhe_plain_create
// and rtfhe_trlwe_mul_plain_batch[_dev] (rtfhe_plain.hip) allocate or launch anything.
#include "rtfhe_plain_plan.h"

#include <cstdio>
#include <string>

#include "../../include/rtfhe.h"

namespace {

int refuse(char* err, size_t err_len, const std::string& msg) {
    if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
    return RTFHE_ERR_INVALID;
}

std::string num(long long v) { return std::to_string(v); }

}  // namespace

extern "C" int rtfhe_plain_weights_plan(int32_t N, const int32_t* w, int32_t n_w, int64_t* wmax, char* err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    if (!w || !wmax) return refuse(err, err_len, "null argument");
    *wmax = 0;
    if (N < 1) return refuse(err, err_len, "N = " + num(N) + " is below 1");
    if (n_w < 1) return refuse(err, err_len, "n_w = " + num(n_w) + " is below 1");
    if ((size_t)n_w > (size_t)0x7fffffff / (size_t)N) return refuse(err, err_len, "n_w * N too large (it must be below 2^31)");
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
    if (err && err_len) err[0] = 0;
    if (!x || !out) return refuse(err, err_len, "null argument");
    if (N < 1) return refuse(err, err_len, "N = " + num(N) + " is below 1");
    if (K < 1 || K > RTFHE_PLAIN_K_MAX) return refuse(err, err_len, "K = " + num(K) + " is outside [1, " + num(RTFHE_PLAIN_K_MAX) + "]");
    const int64_t limit = (int64_t)RTFHE_PLAIN_L1_PER_N * N;
    if (wmax < 0 || wmax > limit / K)      // K * wmax <= limit, without the product (wmax goes up to N * 2^31)
        return refuse(err, err_len, "K * wmax = " + num(K) + " * " + num(wmax) + " is above the exactness domain " + num(RTFHE_PLAIN_L1_PER_N) + " * N = " + num(limit));
    if (n_w < 1) return refuse(err, err_len, "n_w = " + num(n_w) + " is below 1");
    if (n_x < 1) return refuse(err, err_len, "n_x = " + num(n_x) + " is below 1");
    if (count > (size_t)0x7fffffff / (size_t)K) return refuse(err, err_len, "count * K too large (it must be below 2^31)");
    if (count == 0) return 0;
    if (!w_idx_given && n_w < K)
        return refuse(err, err_len, "w_idx NULL: sample 0 reads weights up to " + num(K - 1) + ", the set has " + num(n_w));
    if (!x_idx_given && (size_t)n_x < count * (size_t)K)
        return refuse(err, err_len, "x_idx NULL: sample " + num((long long)(n_x / K)) + " reads rows up to " + num((long long)(n_x / K) * K + K - 1) + ", x has " + num(n_x));
    for (size_t g = 0; g < count; g++)
        for (int32_t k = 0; k < K; k++) {
            if (w_idx && (uint32_t)w_idx[g * K + k] >= (uint32_t)n_w)
                return refuse(err, err_len, "sample " + num((long long)g) + ": w_idx[" + num(k) + "] = " + num(w_idx[g * K + k]) + " is outside [0, " + num(n_w) + ")");
            if (x_idx && (uint32_t)x_idx[g * K + k] >= (uint32_t)n_x)
                return refuse(err, err_len, "sample " + num((long long)g) + ": x_idx[" + num(k) + "] = " + num(x_idx[g * K + k]) + " is outside [0, " + num(n_x) + ")");
        }
    const size_t in_bytes = (size_t)n_x * 2 * (size_t)N * 4, out_bytes = count * 2 * (size_t)N * 4;
    const uintptr_t i0 = (uintptr_t)x, o0 = (uintptr_t)out;
    if (i0 < o0 + out_bytes && o0 < i0 + in_bytes) return refuse(err, err_len, "the output overlaps the TRLWE rows x");
    return 0;
}
