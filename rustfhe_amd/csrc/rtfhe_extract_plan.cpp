// rtfhe_extract_plan.cpp -- host only: the argument checks of TRLWE sample extraction and of its inverse, the packing key switch
// (rtfhe_extract_plan.h), before rtfhe_trlwe_extract_batch[_dev] / rtfhe_trlwe_extract_lvl1_batch[_dev] (rtfhe_extract.hip) and
// rtfhe_pack_batch[_dev] (rtfhe_pack.hip) allocate or launch anything.  Written with rtfhe_plan_kit.hpp: both are a "list or p * stride" rule.
#include "rtfhe_extract_plan.h"

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

extern "C" int rtfhe_extract_plan(int32_t N, int32_t P, const int32_t* coef, int32_t stride, size_t count, const void* in, const void* out,
                                  size_t out_words, int32_t* idx, char* err, size_t err_len) {
    begin(err, err_len);
    if (!in || !out || !idx) return refuse(err, err_len, "null argument");
    if (P < 1 || P > N) return refuse(err, err_len, "P = " + num(P) + " is outside [1, " + num(N) + "]");
    if (!coef && stride < 1) return refuse(err, err_len, "coef NULL: stride = " + num(stride) + " is below 1");
    if (int rc = list_or_stride(coef, stride, P, N, "coef", "stride", idx, err, err_len)) return rc;
    if (!count_fits(count, (size_t)P)) return refuse(err, err_len, "count * P too large (it must be below 2^31)");
    if (rows_overlap(in, count * 2 * (size_t)N * 4, out, count * (size_t)P * out_words * 4)) return refuse(err, err_len, "the output overlaps the TRLWE rows");
    return 0;
}

extern "C" int rtfhe_pack_plan(int32_t N, int32_t P, const int32_t* pos, int32_t rep, size_t count, const void* in, const void* out, int32_t* shift,
                               char* err, size_t err_len) {
    begin(err, err_len);
    if (!in || !out || !shift) return refuse(err, err_len, "null argument");
    if (P < 1 || P > N) return refuse(err, err_len, "P = " + num(P) + " is outside [1, " + num(N) + "]");
    if (rep < 1 || rep > N) return refuse(err, err_len, "rep = " + num(rep) + " is outside [1, " + num(N) + "]");
    if (!count_fits(count, (size_t)P)) return refuse(err, err_len, "count * P too large");
    return list_or_stride(pos, rep, P, 2 * (long long)N, "pos", "rep", shift, err, err_len);
}
