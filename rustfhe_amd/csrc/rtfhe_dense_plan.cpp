// rtfhe_dense_plan.cpp -- host only: the argument checks, the correction words and the launch rule of the lvl0 dense layer (rtfhe_dense_plan.h),
// before rtfhe_dense_create and rtfhe_tlwe_dense_batch[_dev] (rtfhe_dense.hip) allocate or launch anything.
#include "rtfhe_dense_plan.h"

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

namespace {

// 1 <= O, I <= RTFHE_DENSE_MAX, else the message
std::string dims(int32_t O, int32_t I) {
    if (O < 1 || O > RTFHE_DENSE_MAX) return "O = " + num(O) + " is outside [1, " + num(RTFHE_DENSE_MAX) + "]";
    if (I < 1 || I > RTFHE_DENSE_MAX) return "I = " + num(I) + " is outside [1, " + num(RTFHE_DENSE_MAX) + "]";
    return std::string();
}

}  // namespace

extern "C" int rtfhe_dense_weights_plan(const int32_t* W, int32_t O, int32_t I, uint32_t* corr, char* err, size_t err_len) {
    begin(err, err_len);
    if (!W || !corr) return refuse(err, err_len, "null argument");
    const std::string bad = dims(O, I);
    if (!bad.empty()) return refuse(err, err_len, bad);
    for (int32_t o = 0; o < O; o++)
        for (int32_t i = 0; i < I; i++) {
            const int32_t v = W[(size_t)o * I + i];
            if (v < -128 || v > 127) return refuse(err, err_len, "W[" + num(o) + "][" + num(i) + "] = " + num(v) + " is outside [-128, 127]");
        }
    for (int32_t o = 0; o < O; o++) {
        int64_t sum = 0;                          // |sum| <= 65,536 * 128 = 2^23
        for (int32_t i = 0; i < I; i++) sum += W[(size_t)o * I + i];
        corr[o] = (uint32_t)0x80808080u * (uint32_t)(uint64_t)sum;      // 128 * 0x01010101 * sum mod 2^32
    }
    return 0;
}

extern "C" int rtfhe_dense_plan(int32_t n, int32_t O, int32_t I, size_t count, const void* x, const void* out, char* err, size_t err_len) {
    begin(err, err_len);
    if (!x || !out) return refuse(err, err_len, "null argument");
    if (n < 1) return refuse(err, err_len, "n = " + num(n) + " is below 1");
    const std::string bad = dims(O, I);
    if (!bad.empty()) return refuse(err, err_len, bad);
    const size_t words = (size_t)n + 1, widest = (size_t)(I > O ? I : O) * words;       // <= 2^16 * 2^31: no overflow in 64 bits
    if (!count_fits(count, widest)) return refuse(err, err_len, "count * max(I, O) * (n + 1) too large (it must be below 2^31 words)");
    const size_t in_bytes = count * (size_t)I * words * 4, out_bytes = count * (size_t)O * words * 4;
    if (count && rows_overlap(x, in_bytes, out, out_bytes)) return refuse(err, err_len, "the output overlaps the input rows x");
    return 0;
}

extern "C" void rtfhe_dense_launch_shape(int32_t n, int32_t O, int32_t I, size_t count, int32_t cus, rtfhe_dense_shape* s) {
    const int32_t otiles = (O + 15) / 16, cpairs = (n + 1 + 16 * RTFHE_DENSE_CT - 1) / (16 * RTFHE_DENSE_CT);
    s->tiles = otiles >= 4 ? 4 : otiles >= 2 ? 2 : 1;
    s->groups = (otiles + s->tiles - 1) / s->tiles;
    s->cwgs = (cpairs + 3) / 4;
    s->ksteps = (I + 63) / 64;
    s->slices = 1;
    s->steps = s->ksteps;
    const size_t base = count * (size_t)s->groups * (size_t)s->cwgs, want = (size_t)2 * (size_t)(cus < 1 ? 1 : cus);
    if (base == 0 || base >= want || s->ksteps < 4) return;
    size_t slices = (want + base - 1) / base;
    if (slices > (size_t)s->ksteps / 2) slices = (size_t)s->ksteps / 2;
    s->steps = (int32_t)(((size_t)s->ksteps + slices - 1) / slices);
    s->slices = (s->ksteps + s->steps - 1) / s->steps;      // no empty slice
}
