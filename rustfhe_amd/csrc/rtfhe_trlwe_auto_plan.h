/* rtfhe_trlwe_auto_plan.h -- the host-only part of the TRLWE key switch (include/rtfhe.h: rtfhe_trlwe_ksk_keygen, rtfhe_trlwe_ksk_create,
 * rtfhe_trlwe_auto_batch[_dev]): every argument check that needs no context, the inverse exponents the kernel gathers by, and the automorphism's
 * permutation (inline below: rtfhe_keygen.cpp makes rtfhe_trlwe_automorphism and the key's messages with it), with no device call in it
 * (rtfhe_trlwe_auto_plan.cpp).  Internal: rtfhe_trlwe_auto.hip and rtfhe_keygen.cpp call it before
 * anything is allocated, drawn or launched, and tests/c/trlwe_auto_sanitize_main.c walks it under the host sanitizers.  Plain C so that a C host
 * can include it. */
#ifndef RTFHE_TRLWE_AUTO_PLAN_H
#define RTFHE_TRLWE_AUTO_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most steps of one call (the program rides in the launch's arguments, as rot[] of rtfhe_trgsw_rotate_batch does) */
#define RTFHE_TRLWE_AUTO_MAX_STEPS 16
/* the most exponents of one switching key */
#define RTFHE_TRLWE_AUTO_MAX_EXPONENTS 64

/* The rules themselves, in the header: rtfhe_keygen.cpp applies them without linking this unit (as it does with rtfhe_mb_trgsw_count). */
static inline int rtfhe_trlwe_auto_ring_ok(int32_t N) { return N >= 2 && N <= (1 << 20) && (N & (N - 1)) == 0; }
static inline int rtfhe_trlwe_auto_exponent_ok(int32_t N, int32_t t) { return t >= 1 && t < 2 * N && (t & 1); }
/* 0: t[0 .. n_t) is a list a switching key can be made for; 1: N, t or n_t; 2 + e: entry e is even or outside [1, 2N), or repeats an earlier one */
static inline int32_t rtfhe_trlwe_auto_exponents_bad(int32_t N, const int32_t *t, int32_t n_t) {
    if (!rtfhe_trlwe_auto_ring_ok(N) || !t || n_t < 1 || n_t > RTFHE_TRLWE_AUTO_MAX_EXPONENTS) return 1;
    for (int32_t e = 0; e < n_t; e++) {
        if (!rtfhe_trlwe_auto_exponent_ok(N, t[e])) return 2 + e;
        for (int32_t f = 0; f < e; f++)
            if (t[f] == t[e]) return 2 + e;
    }
    return 0;
}
/* sigma_t of one polynomial: in[j] goes to out[j t mod 2N mod N], negated when j t mod 2N >= N.  in and out do not overlap; N and t obey the rules. */
static inline void rtfhe_trlwe_auto_permute(int32_t N, int32_t t, const uint32_t *in, uint32_t *out) {
    const uint32_t mask = (uint32_t)(2 * N - 1);
    for (int32_t j = 0; j < N; j++) {
        const uint32_t q = ((uint32_t)j * (uint32_t)t) & mask;
        out[q & (uint32_t)(N - 1)] = q < (uint32_t)N ? in[j] : 0u - in[j];
    }
}

/* The exponent rules of a switching key, in this order: N a power of two in [2, 2^20]; t non-null; 1 <= n_t <= RTFHE_TRLWE_AUTO_MAX_EXPONENTS;
 * every t[e] odd and in [1, 2N); no exponent twice.
 * Returns 0, or RTFHE_ERR_INVALID with a message naming the entry in err (always terminated; err_len >= 1; err may be null). */
int rtfhe_trlwe_auto_exponents_plan(int32_t N, const int32_t *t, int32_t n_t, char *err, size_t err_len);

/* t^-1 mod 2N for an odd t in [1, 2N), N a power of two; 0 where the arguments break those rules */
int32_t rtfhe_trlwe_auto_inverse(int32_t N, int32_t t);

/* The checks of one call, in this order: entry, x and out non-null; N a power of two in [2, 2^20]; n_t in [1, RTFHE_TRLWE_AUTO_MAX_EXPONENTS];
 * 1 <= n_steps <= RTFHE_TRLWE_AUTO_MAX_STEPS; every entry[k] in [0, n_t); every add[k] in {0, 1} (add may be null: all replace);
 * count <= 2^31 - 1 (a row NUMBER is 32-bit, its offset count * 2N words is formed in size_t: DESIGN.md 6.2); out [count][2][N] is exactly x or
 * shares no byte with it (u32 words; compared as addresses and never dereferenced).  entry and add are HOST arrays in both forms of the call.
 * Returns 0, or RTFHE_ERR_INVALID with a message naming the step in err (always terminated; err_len >= 1; err may be null). */
int rtfhe_trlwe_auto_plan(int32_t N, int32_t n_t, const int32_t *entry, const int32_t *add, int32_t n_steps, size_t count, const void *x,
                          const void *out, char *err, size_t err_len);

#ifdef __cplusplus
}
#endif

#endif
