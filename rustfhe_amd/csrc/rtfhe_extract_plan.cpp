// rtfhe_extract_plan.cpp -- host only: the argument checks of TRLWE sample extraction (rtfhe_extract_plan.h), before
// rtfhe_trlwe_extract_batch[_dev] / rtfhe_trlwe_extract_lvl1_batch[_dev] (rtfhe_extract.hip) allocate or launch anything.
#include "rtfhe_extract_plan.h"

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

extern "C" int rtfhe_extract_plan(int32_t N, int32_t P, const int32_t* coef, int32_t stride, size_t count, const void* in, const void* out,
                                  size_t out_words, int32_t* idx, char* err, size_t err_len) {
    if (err && err_len) err[0] = 0;
    if (!in || !out || !idx) return refuse(err, err_len, "null argument");
    if (P < 1 || P > N) return refuse(err, err_len, "P = " + num(P) + " is outside [1, " + num(N) + "]");
    if (!coef && stride < 1) return refuse(err, err_len, "coef NULL: stride = " + num(stride) + " is below 1");
    for (int32_t p = 0; p < P; p++) {
        const long long v = coef ? (long long)coef[p] : (long long)p * stride;
        if (v < 0 || v >= N)
            return refuse(err, err_len, "sample " + num(p) + ": coef = " + num(v) + " is outside [0, " + num(N) + ")" + (coef ? "" : " (coef NULL: p * stride)"));
        idx[p] = (int32_t)v;
    }
    if (count > (size_t)0x7fffffff / (size_t)P) return refuse(err, err_len, "count * P too large (it must be below 2^31)");
    const size_t in_bytes = count * 2 * (size_t)N * 4, out_bytes = count * (size_t)P * out_words * 4;
    const char *i0 = (const char*)in, *o0 = (const char*)out;
    if ((uintptr_t)i0 < (uintptr_t)o0 + out_bytes && (uintptr_t)o0 < (uintptr_t)i0 + in_bytes) return refuse(err, err_len, "the output overlaps the TRLWE rows");
    return 0;
}
