/* Walks the host-only unit of the seeded lvl0 ciphertexts (rustfhe_amd/csrc/rtfhe_seeded.cpp: the mask rule for rows of length n on the CPU,
 * the seeded lvl0 encryptors, the seeded key-switching key and every argument check of the seeded lvl0 calls) under AddressSanitizer +
 * UndefinedBehaviorSanitizer.  No device is needed: nothing in that unit makes a HIP call.  Every buffer is heap-allocated at exactly the size
 * the header promises, so that an access past it is caught -- a row of n words whose last ChaCha20 block is partial above all; the plan's buffers
 * are addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_seeded_plan.h"

static char err[200];
static const uint32_t seed[8] = {0x03020100u, 0x07060504u, 0x0b0a0908u, 0x0f0e0d0cu, 0x13121110u, 0x17161514u, 0x1b1a1918u, 0x1f1e1d1cu};

static int plan(int32_t what, int32_t n, const void *sd, uint64_t first_row, const void *b, const void *out, size_t rows) {
    memset(err, 'x', sizeof err);
    return rtfhe_tlwe_seeded_plan(what, n, sd, first_row, b, out, rows, err, sizeof err);
}

static void refused(int32_t what, int32_t n, const void *sd, uint64_t first_row, const void *b, const void *out, size_t rows, const char *word) {
    CHECK(plan(what, n, sd, first_row, b, out, rows) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

static uint32_t *words(size_t n) {
    uint32_t *p = malloc(sizeof(uint32_t) * (n ? n : 1));
    CHECK(p);
    memset(p, 0xA5, sizeof(uint32_t) * n);
    return p;
}

/* b - <a, key0> of one lvl0 row */
static uint32_t phase(int n, const int32_t *key, const uint32_t *row) {
    uint32_t s = 0;
    for (int i = 0; i < n; i++) if (key[i]) s += row[i];
    return row[n] - s;
}

static int32_t dist(uint32_t x, uint32_t y) { int32_t d = (int32_t)(x - y); return d < 0 ? -d : d; }

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
/* (b is one word per row: the output is the array that passes 2^32 bytes) */
static int large_plan(size_t rows, const void *b, const void *out) { return plan(RTFHE_TLWE_SEEDED_DEVICE, 767, seed, 5, b, out, rows); }

int main(void) {
    const uint64_t TOP = ~(uint64_t)0;                                              /* 2^64 - 1 */
    const void *b = AT(0x10000000), *out = AT(0x40000000);
    const int HOST = RTFHE_TLWE_SEEDED_HOST, DEV = RTFHE_TLWE_SEEDED_DEVICE, UP = RTFHE_TLWE_SEEDED_UPLOAD;

    /* ---- the plan: accepted at both ends of n and the row numbers ---- */
    CHECK(plan(HOST, 1, seed, 0, b, out, 1) == 0 && err[0] == 0);
    CHECK(plan(HOST, 100000, seed, 0, b, out, 3) == 0);
    CHECK(plan(DEV, 1, seed, 0, b, out, 1) == 0 && plan(DEV, 767, seed, 0xFFFFFFFEull, b, out, 7) == 0);
    CHECK(plan(DEV, 635, seed, TOP - 6 + 1, b, out, 6) == 0);                                       /* first_row + rows = 2^64 */
    CHECK(plan(HOST, 635, seed, TOP, b, out, 1) == 0);
    CHECK(plan(UP, 635, seed, 0, b, NULL, 24576) == 0);                                             /* an upload call's output is the library's own */
    CHECK(plan(DEV, 635, seed, 0, b, AT(0x7000000000000000ull), 0x7fffffff / 40) == 0);             /* the most lanes one launch takes */
    CHECK(plan(DEV, 1, seed, 0, b, AT(0x7000000000000000ull), 0x7fffffff) == 0);
    CHECK(plan(DEV, 635, seed, 0, AT(0x10000004), AT(0x4000000c), 5) == 0);                         /* 4-byte alignment is all it asks */
    CHECK(plan(HOST, 635, seed, 0, AT(0x10000001), AT(0x40000003), 5) == 0);
    CHECK(plan(DEV, 635, seed, 0, b, AT(0x10000000 + 3 * 4), 3) == 0);                              /* out right behind b */
    CHECK(plan(DEV, 635, seed, 0, b, AT(0x10000000 - 3 * 636 * 4), 3) == 0);                        /* and right before it */
    /* ---- refusals: every one is terminated inside err and names what it refuses ---- */
    refused(HOST, 635, NULL, 0, b, out, 1, "null");
    refused(HOST, 635, seed, 0, NULL, out, 1, "null");
    refused(HOST, 635, seed, 0, b, NULL, 1, "null");
    refused(DEV, 635, seed, 0, b, NULL, 1, "null");
    refused(UP, 635, seed, 0, NULL, NULL, 1, "null");
    refused(HOST, 0, seed, 0, b, out, 1, "n = 0");
    refused(HOST, (int32_t)0x80000000, seed, 0, b, out, 1, "n = -2147483648");
    refused(DEV, 768, seed, 0, b, out, 1, "n = 768");
    refused(UP, 768, seed, 0, b, NULL, 1, "n = 768");
    refused(HOST, 635, seed, 0, b, out, 0, "rows = 0");
    refused(DEV, 635, seed, TOP, b, out, 0, "rows = 0");
    refused(HOST, 635, seed, TOP - 6 + 2, b, out, 6, "pass 2^64");                                  /* first_row + rows = 2^64 + 1 */
    refused(HOST, 635, seed, TOP, b, out, 2, "pass 2^64");
    refused(UP, 635, seed, 2, b, NULL, ~(size_t)0, "pass 2^64");
    refused(UP, 635, seed, 1, b, NULL, ~(size_t)0, "too large");                                    /* 2^64 rows exist, but not in one call */
    refused(HOST, 635, seed, 1, b, out, ~(size_t)0, "too large");
    refused(DEV, 635, seed, 0, b, out, 0x7fffffff / 40 + 1, "too large");
    refused(DEV, 1, seed, 0, b, AT(0x7000000000000000ull), 0x80000000ull, "too large");
    refused(UP, 767, seed, 0, b, NULL, 0x7fffffff / 48 + 1, "too large");
    refused(DEV, 635, seed, 0, AT(0x10000002), out, 1, "aligned");
    refused(DEV, 635, seed, 0, b, AT(0x40000001), 1, "aligned");
    refused(HOST, 635, seed, 0, b, b, 3, "overlaps");
    refused(DEV, 635, seed, 0, b, AT(0x10000000 + 3 * 4 - 4), 3, "overlaps");
    refused(DEV, 635, seed, 0, b, AT(0x10000000 - 3 * 636 * 4 + 4), 3, "overlaps");
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_tlwe_seeded_plan(DEV, 768, seed, 0, b, out, 1, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_tlwe_seeded_plan(DEV, 768, seed, 0, b, out, 1, NULL, 0) == RTFHE_ERR_INVALID);
    }

    /* ---- the mask rule: exactly n words per row at every n around a block's end; for n a multiple of 16 the TRLWE rule's known answers ---- */
    {
        static const int ns[] = {1, 15, 16, 17, 31, 32, 33, 635, 766, 767};
        uint32_t *ref = words(3 * 768);
        CHECK(rtfhe_tlwe_mask_expand(768, seed, TOP - 2, ref, 3) == 0);                                /* rows 2^64 - 3 .. 2^64 - 1 */
        for (size_t k = 0; k < sizeof ns / sizeof ns[0]; k++) {
            const int n = ns[k];
            uint32_t *a = words((size_t)3 * n);
            CHECK(rtfhe_tlwe_mask_expand(n, seed, TOP - 2, a, 3) == 0);
            for (int r = 0; r < 3; r++) CHECK(memcmp(a + (size_t)r * n, ref + (size_t)r * 768, sizeof(uint32_t) * (size_t)n) == 0);
            free(a);
        }
        free(ref);
        uint32_t *a = words(1024), *t = words(1024);
        CHECK(rtfhe_tlwe_mask_expand(1024, seed, 5, a, 1) == 0 && rtfhe_mask_expand(1024, seed, 5, t, 1) == 0);
        CHECK(memcmp(a, t, sizeof(uint32_t) * 1024) == 0 && a[1008] == 0x33d19c69u && a[1023] == 0xd526d505u);
        CHECK(rtfhe_tlwe_mask_expand(1024, seed, 0, a, 1) == 0 && a[0] == 0x7d2bfd39u && a[3] == 0x494adcb8u && a[15] == 0x0c415b48u);
        CHECK(rtfhe_tlwe_mask_expand(17, seed, TOP, a, 2) == RTFHE_ERR_INVALID && rtfhe_tlwe_mask_expand(17, seed, 0xFFFFFFFFull, a, 2) == 0);
        CHECK(rtfhe_tlwe_mask_expand(17, NULL, 0, a, 2) == RTFHE_ERR_INVALID && rtfhe_tlwe_mask_expand(17, seed, 0, NULL, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_mask_expand(0, seed, 0, a, 1) == RTFHE_ERR_INVALID && rtfhe_tlwe_mask_expand(17, seed, 0, a, 0) == RTFHE_ERR_INVALID);
        free(a); free(t);
    }

    /* ---- one small encrypt / expand of every kind at n = 21, N = 16, and what it means ---- */
    {
        enum { n = 21, N = 16, ROWS = N * 8 * 3 };
        rtfhe_params p;
        p.n = n; p.N = N; p.nbit = 4; p.l = 3; p.bgbit = 6; p.ks_t = 8; p.ks_basebit = 2;
        int32_t *key0 = malloc(sizeof(int32_t) * n), *key1 = malloc(sizeof(int32_t) * N);
        CHECK(key0 && key1);
        for (int i = 0; i < n; i++) key0[i] = (i * 5 + 1) % 3 == 0;
        for (int i = 0; i < N; i++) key1[i] = (i * 7 + 1) % 3 != 0;
        uint32_t fresh[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const uint8_t bits[3] = {1, 0, 1};
        const uint32_t mu[3] = {0x40000000u, 0x12345678u, 0xC0000000u};
        uint32_t *eb = words(3), *full = words(3 * (n + 1));
        /* bits, production form: rows from 0, a seed from the OS */
        CHECK(rtfhe_tlwe_encrypt_bits_seeded(&p, key0, bits, fresh, eb, 3) == 0);
        CHECK(fresh[0] | fresh[1] | fresh[2] | fresh[3] | fresh[4] | fresh[5] | fresh[6] | fresh[7]);
        CHECK(rtfhe_tlwe_seeded_expand(&p, fresh, 0, eb, full, 3) == 0);
        for (int g = 0; g < 3; g++) CHECK(dist(phase(n, key0, full + g * (n + 1)), bits[g] ? 0x20000000u : 0xE0000000u) < (1 << 21));
        /* torus words, deterministic, at the last rows there are */
        CHECK(rtfhe_tlwe_encrypt_torus_seeded_deterministic(&p, key0, 9, seed, TOP - 2, mu, eb, 3) == 0);
        CHECK(rtfhe_tlwe_encrypt_torus_seeded_deterministic(&p, key0, 9, seed, TOP - 1, mu, eb, 3) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_seeded_expand(&p, seed, TOP - 2, eb, full, 3) == 0);
        for (int g = 0; g < 3; g++) CHECK(dist(phase(n, key0, full + g * (n + 1)), mu[g]) < (1 << 21) && full[g * (n + 1) + n] == eb[g]);
        CHECK(rtfhe_tlwe_encrypt_torus_seeded(&p, key0, mu, fresh, eb, 3) == 0);
        CHECK(rtfhe_tlwe_encrypt_bits_seeded_deterministic(&p, key0, 9, seed, 0xFFFFFFFEull, bits, eb, 3) == 0);
        CHECK(rtfhe_tlwe_seeded_expand(&p, seed, TOP - 1, eb, full, 3) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_seeded_expand(&p, seed, 0, full + 2, full, 3) == RTFHE_ERR_INVALID);          /* b inside out */
        CHECK(rtfhe_tlwe_seeded_expand(NULL, seed, 0, eb, full, 3) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_seeded_expand(&p, seed, 0, eb, full, 0) == RTFHE_ERR_INVALID);
        /* the key-switching key: N * 8 * 3 rows, threads and all */
        uint32_t *kb = words(ROWS), *kfull = words((size_t)ROWS * (n + 1));
        CHECK(rtfhe_ksk_keygen_seeded(&p, key0, key1, fresh, kb) == 0);
        CHECK(rtfhe_ksk_keygen_seeded_deterministic(&p, 6, key0, key1, seed, TOP - ROWS + 1, kb) == 0);
        CHECK(rtfhe_ksk_keygen_seeded_deterministic(&p, 6, key0, key1, seed, TOP - ROWS + 2, kb) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_seeded_expand(&p, seed, TOP - ROWS + 1, kb, kfull, ROWS) == 0);
        for (int i = 0; i < N; i++)                                                                     /* row (i, lv 1, d 2): 3 key1[i] / 2^4 */
            CHECK(dist(phase(n, key0, kfull + (size_t)((i * 8 + 1) * 3 + 2) * (n + 1)), key1[i] ? 3u << 28 : 0u) < (1 << 21));
        key0[1] = 2;
        CHECK(rtfhe_ksk_keygen_seeded(&p, key0, key1, fresh, kb) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_encrypt_bits_seeded(&p, key0, bits, fresh, eb, 3) == RTFHE_ERR_INVALID);
        key0[1] = 0; key1[2] = -1;
        CHECK(rtfhe_ksk_keygen_seeded(&p, key0, key1, fresh, kb) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_encrypt_bits_seeded(&p, NULL, bits, fresh, eb, 3) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_tlwe_encrypt_torus_seeded(NULL, key0, mu, fresh, eb, 3) == RTFHE_ERR_INVALID);
        free(kb); free(kfull); free(eb); free(full); free(key0); free(key1);
    }
    {
        const size_t rows[2] = {1398102 + 3, 5592405 + 3};
        for (int t = 0; t < 2; t++) large_cases(large_plan, rows[t], rows[t] * 4, rows[t] * 3072, 4, "overlaps");
        large_limit(large_plan, (size_t)0x7fffffff / 48, 4, "rows * ceil(n / 16)");
    }
    printf("tlwe seeded sanitizer walk ok\n");
    return 0;
}
