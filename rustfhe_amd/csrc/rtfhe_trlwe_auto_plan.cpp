// rtfhe_trlwe_auto_plan.cpp -- host only: the argument checks of the TRLWE key switch (rtfhe_trlwe_auto_plan.h), before rtfhe_trlwe_ksk_keygen
// (rtfhe_keygen.cpp) draws anything and before rtfhe_trlwe_ksk_create / rtfhe_trlwe_auto_batch[_dev] (rtfhe_trlwe_auto.hip) allocate or launch
// anything; and the inverse exponent the kernel gathers by.  (The automorphism on the CPU, rtfhe_trlwe_automorphism, is rtfhe_keygen.cpp's: a
// client's function, beside the key generator that uses the same permutation from the header.)
#include "rtfhe_trlwe_auto_plan.h"

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

namespace {

bool ring_ok(int32_t N) { return rtfhe_trlwe_auto_ring_ok(N) != 0; }
bool exponent_ok(int32_t N, int32_t t) { return rtfhe_trlwe_auto_exponent_ok(N, t) != 0; }

}  // namespace

extern "C" {

int rtfhe_trlwe_auto_exponents_plan(int32_t N, const int32_t* t, int32_t n_t, char* err, size_t err_len) {
    begin(err, err_len);
    if (!ring_ok(N)) return refuse(err, err_len, "N = " + num(N) + " is not a power of two in [2, 2^20]");
    if (!t) return refuse(err, err_len, "null argument");
    if (n_t < 1 || n_t > RTFHE_TRLWE_AUTO_MAX_EXPONENTS)
        return refuse(err, err_len, "n_t = " + num(n_t) + " is outside [1, " + num(RTFHE_TRLWE_AUTO_MAX_EXPONENTS) + "]");
    for (int32_t e = 0; e < n_t; e++) {
        if (!exponent_ok(N, t[e]))
            return refuse(err, err_len, "entry " + num(e) + ": t = " + num(t[e]) + " is not an odd number in [1, " + num(2ll * N) + ")");
        for (int32_t f = 0; f < e; f++)
            if (t[f] == t[e]) return refuse(err, err_len, "entry " + num(e) + ": t = " + num(t[e]) + " is entry " + num(f) + " already");
    }
    return 0;
}

// Newton's iteration on the 2-adic inverse: x <- x (2 - t x) doubles the correct low bits, and x = t is right to 3 bits (t^2 = 1 mod 8)
int32_t rtfhe_trlwe_auto_inverse(int32_t N, int32_t t) {
    if (!ring_ok(N) || !exponent_ok(N, t)) return 0;
    uint32_t x = (uint32_t)t;
    for (int i = 0; i < 4; i++) x *= 2u - (uint32_t)t * x;      // 3 -> 6 -> 12 -> 24 -> 48 bits; 2N <= 2^21
    return (int32_t)(x & (uint32_t)(2 * N - 1));
}

int rtfhe_trlwe_auto_plan(int32_t N, int32_t n_t, const int32_t* entry, const int32_t* add, int32_t n_steps, size_t count, const void* x,
                          const void* out, char* err, size_t err_len) {
    begin(err, err_len);
    if (!entry || !x || !out) return refuse(err, err_len, "null argument");
    if (!ring_ok(N)) return refuse(err, err_len, "N = " + num(N) + " is not a power of two in [2, 2^20]");
    if (n_t < 1 || n_t > RTFHE_TRLWE_AUTO_MAX_EXPONENTS)
        return refuse(err, err_len, "n_t = " + num(n_t) + " is outside [1, " + num(RTFHE_TRLWE_AUTO_MAX_EXPONENTS) + "]");
    if (n_steps < 1 || n_steps > RTFHE_TRLWE_AUTO_MAX_STEPS)
        return refuse(err, err_len, "n_steps = " + num(n_steps) + " is outside [1, " + num(RTFHE_TRLWE_AUTO_MAX_STEPS) + "]");
    for (int32_t k = 0; k < n_steps; k++) {
        if ((uint32_t)entry[k] >= (uint32_t)n_t)
            return refuse(err, err_len, "step " + num(k) + ": entry = " + num(entry[k]) + " is outside [0, " + num(n_t) + ")");
        if (add && add[k] != 0 && add[k] != 1) return refuse(err, err_len, "step " + num(k) + ": add = " + num(add[k]) + " is neither 0 nor 1");
    }
    if (!count_fits(count, 1)) return refuse(err, err_len, "count too large (it must be below 2^31)");
    const size_t bytes = count * 2 * (size_t)N * 4;
    if (out != x && rows_overlap(x, bytes, out, bytes)) return refuse(err, err_len, "the output overlaps the rows x (it may only be exactly x)");
    return 0;
}

}  // extern "C"
