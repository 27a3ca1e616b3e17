/* Walks the host-only unit of the seeded ciphertexts (rustfhe_amd/csrc/rtfhe_seeded.cpp: the mask rule on the CPU, the seeded encryptors and every
 * argument check of the seeded calls) under AddressSanitizer + UndefinedBehaviorSanitizer.  No device is needed: nothing in that unit makes a HIP
 * call.  Every buffer is heap-allocated at exactly the size the header promises, so that an access past it is caught; the plan's buffers are
 * addresses only and are never dereferenced. */
#include "rtfhe.h"
#include "sanitize_kit.h"
#include "rtfhe_seeded_plan.h"

static char err[200];
static const uint32_t seed[8] = {0x03020100u, 0x07060504u, 0x0b0a0908u, 0x0f0e0d0cu, 0x13121110u, 0x17161514u, 0x1b1a1918u, 0x1f1e1d1cu};

static int plan(int32_t what, int32_t N, const void *sd, uint64_t first_row, const void *b, int32_t group, const void *out, size_t rows) {
    memset(err, 'x', sizeof err);
    return rtfhe_seeded_plan(what, N, sd, first_row, b, group, out, rows, err, sizeof err);
}

static void refused(int32_t what, int32_t N, const void *sd, uint64_t first_row, const void *b, int32_t group, const void *out, size_t rows, const char *word) {
    CHECK(plan(what, N, sd, first_row, b, group, out, rows) == RTFHE_ERR_INVALID);
    CHECK(memchr(err, 0, sizeof err) && strstr(err, word));
}

static uint32_t *words(size_t n) {
    uint32_t *p = malloc(sizeof(uint32_t) * (n ? n : 1));
    CHECK(p);
    memset(p, 0xA5, sizeof(uint32_t) * n);
    return p;
}

/* b - a * s of one TRLWE (negacyclic, binary key) */
static void phase(int N, const int32_t *key, const uint32_t *b, const uint32_t *a, uint32_t *ph) {
    memcpy(ph, b, sizeof(uint32_t) * (size_t)N);
    for (int j = 0; j < N; j++) {
        if (!key[j]) continue;
        for (int k = 0; k < N - j; k++) ph[k + j] -= a[k];
        for (int k = N - j; k < N; k++) ph[k + j - N] += a[k];
    }
}

static int32_t dist(uint32_t x, uint32_t y) { int32_t d = (int32_t)(x - y); return d < 0 ? -d : d; }

/* buffers past 4 GiB and 16 GiB, and the item rule where the bytes are terabytes (sanitize_kit.h: large_cases, large_limit) */
/* (the device form asks for 16-byte alignment first: the shared piece is 16 bytes) */
static int large_plan(size_t rows, const void *b, const void *out) { return plan(RTFHE_SEEDED_DEVICE, 2048, seed, 5, b, 1, out, rows); }

int main(void) {
    const uint64_t TOP = ~(uint64_t)0;                                              /* 2^64 - 1 */
    const void *b = AT(0x10000000), *out = AT(0x40000000);

    /* ---- the plan: accepted at both ends of N, group and the row numbers ---- */
    CHECK(plan(RTFHE_SEEDED_HOST, 16, seed, 0, b, 1, out, 1) == 0 && err[0] == 0);
    CHECK(plan(RTFHE_SEEDED_HOST, 2048, seed, 0, b, 6, out, 18) == 0);
    CHECK(plan(RTFHE_SEEDED_DEVICE, 1024, seed, 0xFFFFFFFEull, b, 1, out, 7) == 0);
    CHECK(plan(RTFHE_SEEDED_DEVICE, 1024, seed, TOP - 6 + 1, b, 6, out, 6) == 0);                  /* first_row + rows = 2^64 */
    CHECK(plan(RTFHE_SEEDED_HOST, 1024, seed, TOP, b, 1, out, 1) == 0);
    CHECK(plan(RTFHE_SEEDED_HOST, 1024, seed, TOP, b, 1, out, 0) == 0);
    CHECK(plan(RTFHE_SEEDED_UPLOAD, 1024, seed, 0, b, 6, NULL, 6) == 0);                           /* an upload call's output is the library's own */
    CHECK(plan(RTFHE_SEEDED_DEVICE, 1024, seed, 0, b, 1, AT(0x7000000000000000ull), 0x7fffffff / 64) == 0);      /* the most lanes one launch takes */
    CHECK(plan(RTFHE_SEEDED_HOST, 1024, seed, 0, b, 1, AT(0x10000000 + 3 * 1024 * 4), 3) == 0);    /* out right behind b */
    CHECK(plan(RTFHE_SEEDED_HOST, 1024, seed, 0, b, 1, AT(0x10000000 - 2 * 3 * 1024 * 4), 3) == 0);   /* and right before it */
    /* ---- refusals: every one is terminated inside err and names what it refuses ---- */
    refused(RTFHE_SEEDED_HOST, 1024, NULL, 0, b, 1, out, 1, "null");
    refused(RTFHE_SEEDED_HOST, 1024, seed, 0, NULL, 1, out, 1, "null");
    refused(RTFHE_SEEDED_HOST, 1024, seed, 0, b, 1, NULL, 1, "null");
    refused(RTFHE_SEEDED_DEVICE, 1024, seed, 0, b, 1, NULL, 1, "null");
    refused(RTFHE_SEEDED_HOST, 0, seed, 0, b, 1, out, 1, "N = 0");
    refused(RTFHE_SEEDED_HOST, 8, seed, 0, b, 1, out, 1, "N = 8");
    refused(RTFHE_SEEDED_HOST, 48, seed, 0, b, 1, out, 1, "N = 48");
    refused(RTFHE_SEEDED_HOST, 4096, seed, 0, b, 1, out, 1, "N = 4096");
    refused(RTFHE_SEEDED_HOST, (int32_t)0x80000000, seed, 0, b, 1, out, 1, "N = -2147483648");
    refused(RTFHE_SEEDED_HOST, 1024, seed, 0, b, 0, out, 6, "group = 0");
    refused(RTFHE_SEEDED_HOST, 1024, seed, 0, b, -6, out, 6, "group = -6");
    refused(RTFHE_SEEDED_HOST, 1024, seed, 0, b, 6, out, 7, "not a multiple");
    refused(RTFHE_SEEDED_UPLOAD, 1024, seed, 0, b, 6, NULL, 5, "not a multiple");
    refused(RTFHE_SEEDED_HOST, 1024, seed, TOP - 6 + 2, b, 6, out, 6, "pass 2^64");                 /* first_row + rows = 2^64 + 1 */
    refused(RTFHE_SEEDED_HOST, 1024, seed, TOP, b, 1, out, 2, "pass 2^64");
    refused(RTFHE_SEEDED_UPLOAD, 1024, seed, 2, b, 1, NULL, ~(size_t)0, "pass 2^64");
    refused(RTFHE_SEEDED_UPLOAD, 1024, seed, 1, b, 1, NULL, ~(size_t)0, "too large");                /* 1 + (2^64 - 1) = 2^64 rows exist, but not in one call */
    refused(RTFHE_SEEDED_DEVICE, 1024, seed, 0, b, 1, out, 0x7fffffff / 64 + 1, "too large");
    refused(RTFHE_SEEDED_UPLOAD, 2048, seed, 0, b, 1, NULL, 0x7fffffff / 128 + 1, "too large");
    refused(RTFHE_SEEDED_DEVICE, 1024, seed, 0, AT(0x10000004), 1, out, 1, "aligned");
    refused(RTFHE_SEEDED_DEVICE, 1024, seed, 0, b, 1, AT(0x40000008), 1, "aligned");
    refused(RTFHE_SEEDED_HOST, 1024, seed, 0, b, 1, b, 3, "overlaps");
    refused(RTFHE_SEEDED_DEVICE, 1024, seed, 0, b, 1, AT(0x10000000 + 3 * 1024 * 4 - 16), 3, "overlaps");
    refused(RTFHE_SEEDED_DEVICE, 1024, seed, 0, b, 1, AT(0x10000000 - 2 * 3 * 1024 * 4 + 16), 3, "overlaps");
    {   /* a message longer than err is cut, not written past it; no err at all is fine too */
        char tiny[8];
        CHECK(rtfhe_seeded_plan(RTFHE_SEEDED_HOST, 4096, seed, 0, b, 1, out, 1, tiny, sizeof tiny) == RTFHE_ERR_INVALID && strlen(tiny) == sizeof tiny - 1);
        CHECK(rtfhe_seeded_plan(RTFHE_SEEDED_HOST, 4096, seed, 0, b, 1, out, 1, NULL, 0) == RTFHE_ERR_INVALID);
    }

    /* ---- the mask rule at the edge row numbers: the known answers of key bytes 00 .. 1f ---- */
    {
        uint32_t *a = words(1024);
        CHECK(rtfhe_mask_expand(1024, seed, 0, a, 1) == 0);
        CHECK(a[0] == 0x7d2bfd39u && a[3] == 0x494adcb8u && a[15] == 0x0c415b48u);
        CHECK(rtfhe_mask_expand(1024, seed, 5, a, 1) == 0);
        CHECK(a[1008] == 0x33d19c69u && a[1023] == 0xd526d505u);
        free(a);
        a = words(2 * 2048);
        CHECK(rtfhe_mask_expand(2048, seed, TOP - 1, a, 2) == 0);                  /* rows 2^64 - 2 and 2^64 - 1 */
        CHECK(a[2048 + 2032] == 0x21be8713u && a[2048 + 2047] == 0x99fc8aa5u);
        CHECK(rtfhe_mask_expand(2048, seed, TOP, a, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_mask_expand(2048, seed, 0xFFFFFFFFull, a, 2) == 0);            /* the low word carries between the two rows */
        CHECK(rtfhe_mask_expand(2048, NULL, 0, a, 2) == RTFHE_ERR_INVALID && rtfhe_mask_expand(2048, seed, 0, NULL, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_mask_expand(100, seed, 0, a, 1) == RTFHE_ERR_INVALID);
        free(a);
    }

    /* ---- one small encrypt / expand of every kind at N = 16, and what it means ---- */
    {
        enum { N = 16, L = 3, ROWS = 2 * L };
        rtfhe_params p;
        p.n = 2; p.N = N; p.nbit = 4; p.l = L; p.bgbit = 6; p.ks_t = 8; p.ks_basebit = 2;
        int32_t *key1 = malloc(sizeof(int32_t) * N), *key0 = malloc(sizeof(int32_t) * 2);
        CHECK(key1 && key0);
        for (int i = 0; i < N; i++) key1[i] = (i * 7 + 1) % 3 == 0;
        key0[0] = 1; key0[1] = 0;
        uint32_t fresh[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        /* TRLWE rows, production form: rows from 0, a seed from the OS */
        uint32_t *mu = words(2 * N), *bt = words(2 * N), *full = words(2 * 2 * N), *ph = words(N);
        for (int i = 0; i < 2 * N; i++) mu[i] = (uint32_t)i * 0x01000000u;
        CHECK(rtfhe_trlwe_encrypt_torus_seeded(&p, key1, mu, fresh, bt, 2) == 0);
        CHECK(fresh[0] | fresh[1] | fresh[2] | fresh[3] | fresh[4] | fresh[5] | fresh[6] | fresh[7]);
        CHECK(rtfhe_seeded_expand(&p, fresh, 0, bt, 1, full, 2) == 0);
        for (int g = 0; g < 2; g++) {
            phase(N, key1, full + g * 2 * N, full + g * 2 * N + N, ph);
            for (int i = 0; i < N; i++) CHECK(dist(ph[i], mu[g * N + i]) < (1 << 12));
        }
        /* ... deterministic, at the last rows there are */
        CHECK(rtfhe_trlwe_encrypt_torus_seeded_deterministic(&p, key1, 9, seed, TOP - 1, mu, bt, 2) == 0);
        CHECK(rtfhe_trlwe_encrypt_torus_seeded_deterministic(&p, key1, 9, seed, TOP, mu, bt, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_seeded_expand(&p, seed, TOP - 1, bt, 1, full, 2) == 0);
        phase(N, key1, full + 2 * N, full + 3 * N, ph);
        for (int i = 0; i < N; i++) CHECK(dist(ph[i], mu[N + i]) < (1 << 12));
        CHECK(rtfhe_seeded_expand(&p, seed, TOP - 1, bt, 2, full, 2) == 0);         /* the same rows as one group of two: b b a a */
        CHECK(memcmp(full, bt, sizeof(uint32_t) * 2 * N) == 0);
        CHECK(rtfhe_seeded_expand(&p, seed, 0, bt, 2, full, 1) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_seeded_expand(&p, seed, 0, full, 1, full, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_seeded_expand(NULL, seed, 0, bt, 1, full, 2) == RTFHE_ERR_INVALID);
        free(full);
        /* a TRGSW sample of bit 1 and of a polynomial: row 0's phase is the message / Bg */
        uint32_t *bg = words(ROWS * N), *gfull = words(2 * ROWS * N);
        uint8_t one = 1;
        CHECK(rtfhe_trgsw_encrypt_bits_seeded(&p, key1, &one, fresh, bg, 1) == 0);
        CHECK(rtfhe_seeded_expand(&p, fresh, 0, bg, ROWS, gfull, ROWS) == 0);
        phase(N, key1, gfull, gfull + ROWS * N, ph);
        CHECK(dist(ph[0], 1u << 26) < (1 << 12) && dist(ph[1], 0) < (1 << 12));
        CHECK(rtfhe_trgsw_encrypt_bits_seeded_deterministic(&p, key1, 3, seed, TOP - ROWS + 1, &one, bg, 1) == 0);
        CHECK(rtfhe_trgsw_encrypt_bits_seeded_deterministic(&p, key1, 3, seed, TOP - ROWS + 2, &one, bg, 1) == RTFHE_ERR_INVALID);
        int32_t *pm = malloc(sizeof(int32_t) * N);
        CHECK(pm);
        for (int i = 0; i < N; i++) pm[i] = i - 8;
        CHECK(rtfhe_trgsw_encrypt_polys_seeded(&p, key1, pm, fresh, bg, 1) == 0);
        CHECK(rtfhe_trgsw_encrypt_polys_seeded_deterministic(&p, key1, 4, seed, 0xFFFFFFFEull, pm, bg, 1) == 0);
        CHECK(rtfhe_seeded_expand(&p, seed, 0xFFFFFFFEull, bg, ROWS, gfull, ROWS) == 0);
        phase(N, key1, gfull + N, gfull + (ROWS + 1) * N, ph);                      /* gadget position 1: mu * 2^20 */
        for (int i = 0; i < N; i++) CHECK(dist(ph[i], (uint32_t)pm[i] << 20) < (1 << 12));
        free(pm); free(bg); free(gfull);
        /* the packing key: n * 8 * 3 rows, threads and all */
        uint32_t *bp = words((size_t)2 * 8 * 3 * N), *pfull = words((size_t)2 * 2 * 8 * 3 * N);
        CHECK(rtfhe_packing_keygen_seeded(&p, key0, key1, fresh, bp) == 0);
        CHECK(rtfhe_packing_keygen_seeded_deterministic(&p, 6, key0, key1, seed, TOP - 48 + 1, bp) == 0);
        CHECK(rtfhe_packing_keygen_seeded_deterministic(&p, 6, key0, key1, seed, TOP - 48 + 2, bp) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_seeded_expand(&p, seed, TOP - 48 + 1, bp, 1, pfull, 48) == 0);
        phase(N, key1, pfull + (size_t)(2 * 2 + 1) * 2 * N, pfull + (size_t)(2 * 2 + 1) * 2 * N + N, ph);      /* row (0, lv 1, d 2): 3 / 2^4 */
        CHECK(dist(ph[0], 3u << 28) < (1 << 12) && dist(ph[5], 0) < (1 << 12));
        key0[1] = 2;
        CHECK(rtfhe_packing_keygen_seeded(&p, key0, key1, fresh, bp) == RTFHE_ERR_INVALID);
        key1[2] = -1;
        CHECK(rtfhe_trlwe_encrypt_torus_seeded(&p, key1, mu, fresh, bt, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_trlwe_encrypt_torus_seeded(&p, NULL, mu, fresh, bt, 2) == RTFHE_ERR_INVALID);
        CHECK(rtfhe_trgsw_encrypt_bits_seeded(NULL, key1, &one, fresh, bt, 1) == RTFHE_ERR_INVALID);
        free(bp); free(pfull); free(mu); free(bt); free(ph); free(key1); free(key0);
    }
    for (size_t rows = ((size_t)1 << 19) + 3; rows <= ((size_t)1 << 21) + 3; rows += ((size_t)1 << 21) - ((size_t)1 << 19))
        large_cases(large_plan, rows, rows * 8192, rows * 16384, 16, "overlaps");
    large_limit(large_plan, (size_t)0x7fffffff / 128, 8192, "rows * N / 16");
    printf("seeded sanitizer walk ok\n");
    return 0;
}
