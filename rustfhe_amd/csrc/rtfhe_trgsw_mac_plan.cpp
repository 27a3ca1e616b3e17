// rtfhe_trgsw_mac_plan.cpp -- host only: the argument checks of the TRLWE x TRGSW multiply-accumulate (rtfhe_trgsw_mac_plan.h), before
// rtfhe_trlwe_mul_trgsw_batch[_dev] (rtfhe_trgsw_mac.hip) allocates or launches anything.
#include "rtfhe_trgsw_mac_plan.h"

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

extern "C" int rtfhe_trgsw_mac_plan(int32_t N, int32_t n_sel, int32_t K, int32_t s_idx_given, const int32_t* s_idx, int32_t n_x, int32_t x_idx_given,
                                    const int32_t* x_idx, size_t count, const void* x, const void* out, char* err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    if (!x || !out) return refuse(err, err_len, "null argument");
    if (N < 1) return refuse(err, err_len, "N = " + num(N) + " is below 1");
    if (K < 1 || K > RTFHE_TRGSW_MAC_K_MAX) return refuse(err, err_len, "K = " + num(K) + " is outside [1, " + num(RTFHE_TRGSW_MAC_K_MAX) + "]");
    if (n_sel < 1) return refuse(err, err_len, "n_sel = " + num(n_sel) + " is below 1");
    if (n_x < 1) return refuse(err, err_len, "n_x = " + num(n_x) + " is below 1");
    if (count > (size_t)0x7fffffff / (size_t)K) return refuse(err, err_len, "count * K too large (it must be below 2^31)");
    if (count == 0) return 0;
    if (!s_idx_given && (size_t)n_sel < count * (size_t)K)
        return refuse(err, err_len, "s_idx NULL: sample " + num((long long)(n_sel / K)) + " reads selectors up to " + num((long long)(n_sel / K) * K + K - 1) +
                                        ", the set has " + num(n_sel));
    if (!x_idx_given && (size_t)n_x < count * (size_t)K)
        return refuse(err, err_len, "x_idx NULL: sample " + num((long long)(n_x / K)) + " reads rows up to " + num((long long)(n_x / K) * K + K - 1) + ", x has " + num(n_x));
    for (size_t g = 0; g < count; g++)
        for (int32_t k = 0; k < K; k++) {
            if (s_idx && (uint32_t)s_idx[g * K + k] >= (uint32_t)n_sel)
                return refuse(err, err_len, "sample " + num((long long)g) + ": s_idx[" + num(k) + "] = " + num(s_idx[g * K + k]) + " is outside [0, " + num(n_sel) + ")");
            if (x_idx && (uint32_t)x_idx[g * K + k] >= (uint32_t)n_x)
                return refuse(err, err_len, "sample " + num((long long)g) + ": x_idx[" + num(k) + "] = " + num(x_idx[g * K + k]) + " is outside [0, " + num(n_x) + ")");
        }
    const size_t in_bytes = (size_t)n_x * 2 * (size_t)N * 4, out_bytes = count * 2 * (size_t)N * 4;
    const uintptr_t i0 = (uintptr_t)x, o0 = (uintptr_t)out;
    if (i0 < o0 + out_bytes && o0 < i0 + in_bytes) return refuse(err, err_len, "the output overlaps the TRLWE rows x");
    return 0;
}
