// rtfhe_mb_plan.cpp -- see rtfhe_mb_plan.h.  Host only, no HIP call: compiles under a plain C++17 compiler (tests/c/mb_sanitize_main.c).
#include "rtfhe_mb_plan.h"

#include <cmath>

#include "rtfhe_plan_kit.hpp"

using namespace rtfhe_plan;

namespace {

bool g_ok(int32_t g) { return g >= RTFHE_MB_G_MIN && g <= RTFHE_MB_G_MAX; }
std::string g_refusal(int32_t g) { return "g = " + num(g) + " is outside [" + num(RTFHE_MB_G_MIN) + ", " + num(RTFHE_MB_G_MAX) + "]"; }

}  // namespace

extern "C" {

size_t rtfhe_mbk_words(const rtfhe_params* p, int32_t g) {
    if (!p || p->N < 1 || p->l < 1) return 0;
    const int64_t t = rtfhe_mb_trgsw_count(p->n, g);
    return t < 0 ? 0 : (size_t)t * 2 * 2 * (size_t)p->l * (size_t)p->N;
}

// W[t] = exp(i pi t / N), t in [0, 2N): (cos, sin) of the double pi * t / N.  W[0] = (1, 0) exactly.
int rtfhe_mb_roots(int32_t N, double* out) {
    if (!out || N < 2 || N > (1 << 20) || (N & (N - 1))) return RTFHE_ERR_INVALID;
    const double pi = 3.14159265358979323846;
    for (int32_t t = 0; t < 2 * N; t++) {
        const double x = pi * (double)t / (double)N;
        out[2 * t] = std::cos(x);
        out[2 * t + 1] = std::sin(x);
    }
    return 0;
}

// Spectrum point p = m * 64 + lane of the canonical [R][64] lane order (R = N / 128) is position k = lane * R + m of the transform's own output
// order, where the forward transform leaves the polynomial's value at W[q], q = 4 * bitreverse(k, log2(N / 2)) + 1.
int rtfhe_mb_point_exponents(int32_t N, int32_t* out) {
    if (!out || N < 128 || N > (1 << 20) || (N & (N - 1))) return RTFHE_ERR_INVALID;
    const int32_t P = N / 2, R = P / 64;
    int bits = 0;
    while ((1 << bits) < P) bits++;
    for (int32_t p = 0; p < P; p++) {
        const int32_t m = p >> 6, lane = p & 63, k = lane * R + m;
        int32_t rev = 0;
        for (int b = 0; b < bits; b++) rev |= ((k >> b) & 1) << (bits - 1 - b);
        out[p] = 4 * rev + 1;
    }
    return 0;
}

int rtfhe_mb_key_plan(int32_t n, int32_t N, int32_t l, int32_t g, const void* words, char* err, size_t err_len) {
    begin(err, err_len);
    if (!words) return refuse(err, err_len, "null argument");
    if (!g_ok(g)) return refuse(err, err_len, g_refusal(g));
    if (n < 1) return refuse(err, err_len, "n = " + num(n) + " is below 1");
    if (N != 1024 && N != 2048) return refuse(err, err_len, "N = " + num(N) + ": the multi-bit kernels exist at N = 1024 and 2048");
    if (l < 1) return refuse(err, err_len, "l = " + num(l) + " is below 1");
    if (!count_fits((size_t)rtfhe_mb_trgsw_count(n, g), (size_t)4 * (size_t)l)) return refuse(err, err_len, "the key holds too many polynomials (2^31 or more)");
    return 0;
}

int rtfhe_mb_call_plan(int32_t n, int32_t g, size_t count, const int32_t* lut_idx, int32_t n_lut, const void* tlwe, const void* out, char* err,
                       size_t err_len) {
    begin(err, err_len);
    if (!tlwe || !out) return refuse(err, err_len, "null argument");
    if (!g_ok(g)) return refuse(err, err_len, g_refusal(g));
    if (n < 1) return refuse(err, err_len, "n = " + num(n) + " is below 1");
    if (!count_fits(count, 1)) return refuse(err, err_len, "count too large");
    if (n_lut < 1) return refuse(err, err_len, "n_lut = " + num(n_lut) + " is below 1");
    if (lut_idx)
        for (size_t i = 0; i < count; i++)
            if ((uint32_t)lut_idx[i] >= (uint32_t)n_lut)
                return refuse(err, err_len, "lut_idx[" + num((long long)i) + "] = " + num(lut_idx[i]) + " is outside [0, " + num(n_lut) + ")");
    return 0;
}

}  // extern "C"
