// rtfhe_plan_kit.hpp -- header only, host only, no HIP header: what the argument checks of every entry family are written with, each rule stated
// once ("the plan kit").  The host-only plan units (rtfhe_*_plan.cpp, rtfhe_seeded.cpp) are built on it and compile with it under
// a plain C++17 compiler, as the sanitizer walks under tests/c/ build them; rtfhe_cmux_tree.hip takes rows_overlap from it.
// A plan function opens with begin(err, err_len) and returns 0 or refuse(...): RTFHE_ERR_INVALID with its message in err, always terminated and
// cut to err_len; err may be null.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>

#include "../../include/rtfhe.h"

namespace rtfhe_plan {

inline int refuse(char* err, size_t err_len, const std::string& msg) {
    if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
    return RTFHE_ERR_INVALID;
}

inline std::string num(long long v) { return std::to_string(v); }

// no message yet
inline void begin(char* err, size_t err_len) { if (err && err_len) err[0] = 0; }

// do in [in_bytes] and out [out_bytes] share a byte?  Compared as integers: the buffers may be addresses only and are never dereferenced.
inline bool rows_overlap(const void* in, size_t in_bytes, const void* out, size_t out_bytes) {
    const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
    return i0 < o0 + out_bytes && o0 < i0 + in_bytes;
}

// count * per_item stays below 2^31 (what one launch numbers in 32 bits), without the product; per_item >= 1
inline bool count_fits(size_t count, size_t per_item) { return count <= (size_t)0x7fffffff / per_item; }

// P values, each in [0, bound): the caller's list, or p * stride where it is null.  They go to dst[0 .. P).  list_noun / stride_noun: "coef" /
// "stride", "pos" / "rep".
inline int list_or_stride(const int32_t* list, int32_t stride, int32_t P, long long bound, const char* list_noun, const char* stride_noun, int32_t* dst,
                          char* err, size_t err_len) {
    for (int32_t p = 0; p < P; p++) {
        const long long v = list ? (long long)list[p] : (long long)p * stride;
        if (v < 0 || v >= bound)
            return refuse(err, err_len, "sample " + num(p) + ": " + list_noun + " = " + num(v) + " is outside [0, " + num(bound) + ")" +
                                            (list ? std::string() : std::string(" (") + list_noun + " NULL: p * " + stride_noun + ")"));
        dst[p] = (int32_t)v;
    }
    return 0;
}

// One index array [count][K] of a call that sums K terms per sample, into `n` items of `holder` ("the set", "x").  given: the caller passed one
// (idx: its host form, null in the _dev forms, whose arrays the kernel checks).  Not given, sample g reads items g * K .. g * K + K - 1 -- or,
// shared, every sample items 0 .. K - 1.
struct TermIdx { const char* name; const char* reads; const char* holder; int32_t n; bool given; const int32_t* idx; bool shared; };

// "idx NULL needs count * K entries" (shared: K)
inline int idx_null_ready(const TermIdx& t, size_t count, int32_t K, char* err, size_t err_len) {
    if (t.given || (size_t)t.n >= (t.shared ? 1 : count) * (size_t)K) return 0;
    const long long first = t.shared ? 0 : (long long)(t.n / K);      // the first sample that reads past the end
    return refuse(err, err_len, std::string(t.name) + " NULL: sample " + num(first) + " reads " + t.reads + " up to " + num(first * K + K - 1) + ", " + t.holder +
                                    " has " + num(t.n));
}

// every entry of both host arrays in [0, n), sample by sample: a's entry k before b's
inline int idx_walk(const TermIdx& a, const TermIdx& b, size_t count, int32_t K, char* err, size_t err_len) {
    if (!a.idx && !b.idx) return 0;      // the _dev forms: nothing to walk (count * K goes up to 2^31 - 1: seconds of empty iterations)
    for (size_t g = 0; g < count; g++)
        for (int32_t k = 0; k < K; k++)
            for (const TermIdx* t : {&a, &b})
                if (t->idx && (uint32_t)t->idx[g * K + k] >= (uint32_t)t->n)
                    return refuse(err, err_len, "sample " + num((long long)g) + ": " + t->name + "[" + num(k) + "] = " + num(t->idx[g * K + k]) + " is outside [0, " +
                                                    num(t->n) + ")");
    return 0;
}

// What the two sums of products over TRLWE rows check -- TRLWE x plain (small = the plain set, shared where no w_idx is given) and TRLWE x TRGSW
// (small = the selector set): the head up to the K range, then, behind whatever the caller checks in between, the tail.
inline int terms_head(int32_t N, int32_t K, int32_t K_max, const void* x, const void* out, char* err, size_t err_len) {
    begin(err, err_len);
    if (!x || !out) return refuse(err, err_len, "null argument");
    if (N < 1) return refuse(err, err_len, "N = " + num(N) + " is below 1");
    if (K < 1 || K > K_max) return refuse(err, err_len, "K = " + num(K) + " is outside [1, " + num(K_max) + "]");
    return 0;
}
// (n_small_name: "n_w", "n_sel")
inline int terms_tail(int32_t N, int32_t K, const char* n_small_name, const TermIdx& small, const TermIdx& x_idx, size_t count, const void* x, const void* out,
                      char* err, size_t err_len) {
    if (small.n < 1) return refuse(err, err_len, std::string(n_small_name) + " = " + num(small.n) + " is below 1");
    if (x_idx.n < 1) return refuse(err, err_len, "n_x = " + num(x_idx.n) + " is below 1");
    if (!count_fits(count, (size_t)K)) return refuse(err, err_len, "count * K too large (it must be below 2^31)");
    if (count == 0) return 0;
    if (int rc = idx_null_ready(small, count, K, err, err_len)) return rc;
    if (int rc = idx_null_ready(x_idx, count, K, err, err_len)) return rc;
    if (int rc = idx_walk(small, x_idx, count, K, err, err_len)) return rc;
    const size_t row = 2 * (size_t)N * 4;
    if (rows_overlap(x, (size_t)x_idx.n * row, out, count * row)) return refuse(err, err_len, "the output overlaps the TRLWE rows x");
    return 0;
}

}  // namespace rtfhe_plan
