// rtfhe_seeded.cpp -- host only: seeded ciphertexts (include/rtfhe.h, "seeded ciphertexts" of ring rows and "seeded lvl0 ciphertexts").  The mask
// rule on the CPU (rtfhe_mask_expand, rtfhe_seeded_expand, rtfhe_tlwe_mask_expand, rtfhe_tlwe_seeded_expand: the oracles of k_seeded_expand and
// k_tlwe_seeded_expand and the path of a server without this library's GPU side), the seeded encryptors, the seeded packing and key-switching
// keys, and the argument checks of every seeded call, device calls included (rtfhe_seeded_plan.h).  No HIP call in this unit.
// Every row is made by the encryptor core of rtfhe_encrypt.hpp, the one rtfhe_keygen.cpp's unseeded entry points run, with a SeedMask where
// those hand it a DrawnMask: the mask is the ChaCha20 keystream of the public seed, all 32 bits of every word, and never the generator the
// noise comes from; noise and message words are the core's.
// What is refused: a non-binary key (lvl0 encryptors too, where the unseeded ones take any non-zero word as 1); for ring rows N outside
// [16, 2048] (the unseeded entry points need only valid(p)); rows beyond 2^64.  count = 0 is a no-op of the encryptors; rows = 0 is refused by
// rtfhe_tlwe_seeded_plan.
#include "rtfhe_seeded_plan.h"

#include "rtfhe_encrypt.hpp"
#include "rtfhe_plan_kit.hpp"

namespace {

using namespace rtfhe_encrypt;
using namespace rtfhe_plan;

std::string row_range(uint64_t first_row, size_t rows) {
    return "rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " + std::to_string(rows) + ") pass 2^64";
}

bool ring_ok(int32_t N) { return N >= 16 && N <= 2048 && (N & (N - 1)) == 0; }

// what every seeded encryptor asks first: a valid parameter set (ring rows: one whose ring the mask rule covers), its pointers, count objects of
// rows_each rows that exist.  The binary keys are the caller's to check, once p is known to be valid.
bool ready(const rtfhe_params* p, bool ring, const void* key, const void* in, const uint32_t* seed, const void* b, uint64_t first_row, size_t count,
           size_t rows_each) {
    if (!valid(p) || (ring && !ring_ok(p->N)) || !key || !in || !seed || !b) return false;
    if (rows_each && count > (size_t)-1 / rows_each) return false;
    return rows_ok(first_row, count * rows_each);
}
bool lvl1_ready(const rtfhe_params* p, const int32_t* key1, const void* in, const uint32_t* seed, const void* b, uint64_t first_row, size_t count,
                size_t rows_each) {
    return ready(p, true, key1, in, seed, b, first_row, count, rows_each) && binary(key1, p->N);
}
bool lvl0_ready(const rtfhe_params* p, const int32_t* key0, const void* in, const uint32_t* seed, const void* b, uint64_t first_row, size_t count) {
    return ready(p, false, key0, in, seed, b, first_row, count, 1) && binary(key0, p->n);
}
// rtfhe_packing_keygen_seeded* refuse ks parameters other than (8, 2), as rtfhe_packing_keygen* do
bool packing_ready(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, const uint32_t* seed, const void* b, uint64_t first_row) {
    return lvl1_ready(p, key1, key0, seed, b, 0, 0, 0) && p->ks_t == 8 && p->ks_basebit == 2 && binary(key0, p->n) &&
           rows_ok(first_row, (size_t)p->n * digit_row_count(p));
}
bool ksk_ready(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, const uint32_t* seed, const void* b, uint64_t first_row) {
    return ready(p, false, key0, key1, seed, b, 0, 0, 0) && rows_ok(first_row, (size_t)p->N * digit_row_count(p)) && binary(key0, p->n) &&
           binary(key1, p->N);
}

size_t trgsw_rows_each(const rtfhe_params* p) { return p ? (size_t)2 * p->l : 0; }

}  // namespace

extern "C" {

int rtfhe_seeded_plan(int32_t what, int32_t N, const void* seed, uint64_t first_row, const void* b, int32_t group, const void* out, size_t rows, char* err,
                      size_t err_len) {
    begin(err, err_len);
    const bool upload = what == RTFHE_SEEDED_UPLOAD;
    if (!seed || !b || (!upload && !out)) return refuse(err, err_len, "null argument");
    if (!ring_ok(N)) return refuse(err, err_len, "N = " + num(N) + " is not a power of two in [16, 2048]");
    if (group < 1) return refuse(err, err_len, "group = " + num(group) + " is below 1");
    if (rows % (size_t)group) return refuse(err, err_len, "rows = " + std::to_string(rows) + " is not a multiple of group = " + num(group));
    if (!rows_ok(first_row, rows)) return refuse(err, err_len, row_range(first_row, rows));
    if (what != RTFHE_SEEDED_HOST && !count_fits(rows, (size_t)(N / 16))) return refuse(err, err_len, "rows * N / 16 too large (it must be below 2^31)");
    if (upload) return 0;
    const uintptr_t i0 = (uintptr_t)b, o0 = (uintptr_t)out;
    if (what == RTFHE_SEEDED_DEVICE && ((i0 | o0) & 15)) return refuse(err, err_len, "d_b and d_out must be 16-byte aligned");
    const size_t in_bytes = rows * (size_t)N * 4;
    if (rows_overlap(b, in_bytes, out, 2 * in_bytes)) return refuse(err, err_len, "the output overlaps the b rows");
    return 0;
}

int rtfhe_tlwe_seeded_plan(int32_t what, int32_t n, const void* seed, uint64_t first_row, const void* b, const void* out, size_t rows, char* err,
                           size_t err_len) {
    begin(err, err_len);
    const bool upload = what == RTFHE_TLWE_SEEDED_UPLOAD, host = what == RTFHE_TLWE_SEEDED_HOST;
    if (!seed || !b || (!upload && !out)) return refuse(err, err_len, "null argument");
    if (n < 1 || (!host && n > 767)) return refuse(err, err_len, "n = " + num(n) + (host ? " is below 1" : " is outside [1, 767]"));
    if (rows < 1) return refuse(err, err_len, "rows = 0: a seeded lvl0 object has at least one row");
    if (!rows_ok(first_row, rows)) return refuse(err, err_len, row_range(first_row, rows));
    const size_t w = (size_t)n + 1, nb = ((size_t)n + 15) / 16;
    if (!host && !count_fits(rows, nb)) return refuse(err, err_len, "rows * ceil(n / 16) too large (it must be below 2^31)");
    if (host && rows > ((size_t)-1 / 4) / w) return refuse(err, err_len, "rows * (n + 1) words too large");
    if (upload) return 0;
    const uintptr_t i0 = (uintptr_t)b, o0 = (uintptr_t)out;
    if (what == RTFHE_TLWE_SEEDED_DEVICE && ((i0 | o0) & 3)) return refuse(err, err_len, "d_b and d_out must be 4-byte aligned");
    if (rows_overlap(b, rows * 4, out, rows * w * 4)) return refuse(err, err_len, "the output overlaps the b words");
    return 0;
}

// ---- the mask rule on the CPU ----
int rtfhe_mask_expand(int32_t N, const uint32_t* seed, uint64_t first_row, uint32_t* a, size_t rows) {
    if (!seed || !a || !ring_ok(N) || !rows_ok(first_row, rows)) return RTFHE_ERR_INVALID;
    for (size_t r = 0; r < rows; r++) mask_row(N, seed, first_row + r, a + r * (size_t)N);
    return 0;
}

int rtfhe_seeded_expand(const rtfhe_params* p, const uint32_t* seed, uint64_t first_row, const uint32_t* b, int32_t group, uint32_t* out, size_t rows) {
    if (!p) return RTFHE_ERR_INVALID;
    if (int rc = rtfhe_seeded_plan(RTFHE_SEEDED_HOST, p->N, seed, first_row, b, group, out, rows, nullptr, 0)) return rc;
    const size_t N = (size_t)p->N, G = (size_t)group;
    for (size_t r = 0; r < rows; r++) {
        uint32_t* ob = out + ((r / G) * 2 * G + r % G) * N;
        std::memcpy(ob, b + r * N, N * 4);
        mask_row(p->N, seed, first_row + r, ob + G * N);
    }
    return 0;
}

int rtfhe_tlwe_mask_expand(int32_t n, const uint32_t* seed, uint64_t first_row, uint32_t* a, size_t rows) {
    if (!seed || !a || n < 1 || rows < 1 || !rows_ok(first_row, rows) || rows > ((size_t)-1 / 4) / (size_t)n) return RTFHE_ERR_INVALID;
    for (size_t r = 0; r < rows; r++) mask_row(n, seed, first_row + r, a + r * (size_t)n);
    return 0;
}

int rtfhe_tlwe_seeded_expand(const rtfhe_params* p, const uint32_t* seed, uint64_t first_row, const uint32_t* b, uint32_t* out, size_t rows) {
    if (!p) return RTFHE_ERR_INVALID;
    if (int rc = rtfhe_tlwe_seeded_plan(RTFHE_TLWE_SEEDED_HOST, p->n, seed, first_row, b, out, rows, nullptr, 0)) return rc;
    const size_t n = (size_t)p->n;
    for (size_t r = 0; r < rows; r++) {
        mask_row(p->n, seed, first_row + r, out + r * (n + 1));
        out[r * (n + 1) + n] = b[r];
    }
    return 0;
}

// ---- production: the mask seed and the noise key are two draws from the OS CSPRNG; rows are numbered from 0 ----
int rtfhe_trlwe_encrypt_torus_seeded(const rtfhe_params* p, const int32_t* key1, const uint32_t* mu, uint32_t* seed, uint32_t* b, size_t count) {
    if (!lvl1_ready(p, key1, mu, seed, b, 0, count, 1)) return RTFHE_ERR_INVALID;
    return production(seed, [&](Rng& r) { return encrypt_trlwe(r, SeedMask{seed, 0}, p, key1, mu, b, count); });
}

int rtfhe_trgsw_encrypt_bits_seeded(const rtfhe_params* p, const int32_t* key1, const uint8_t* bits, uint32_t* seed, uint32_t* b, size_t count) {
    if (!lvl1_ready(p, key1, bits, seed, b, 0, count, trgsw_rows_each(p))) return RTFHE_ERR_INVALID;
    return production(seed, [&](Rng& r) { return encrypt_trgsw_bits(r, SeedMask{seed, 0}, p, key1, bits, b, count); });
}

int rtfhe_trgsw_encrypt_polys_seeded(const rtfhe_params* p, const int32_t* key1, const int32_t* mu, uint32_t* seed, uint32_t* b, size_t count) {
    if (!lvl1_ready(p, key1, mu, seed, b, 0, count, trgsw_rows_each(p))) return RTFHE_ERR_INVALID;
    return production(seed, [&](Rng& r) { return encrypt_trgsw_polys(r, SeedMask{seed, 0}, p, key1, mu, b, count); });
}

int rtfhe_packing_keygen_seeded(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* seed, uint32_t* b) {
    if (!packing_ready(p, key0, key1, seed, b, 0)) return RTFHE_ERR_INVALID;
    return production_source(seed, [&](const Source& src) { return packing_keygen(p, src, SeedMask{seed, 0}, key0, key1, b); });
}

int rtfhe_tlwe_encrypt_bits_seeded(const rtfhe_params* p, const int32_t* key0, const uint8_t* bits, uint32_t* seed, uint32_t* b, size_t count) {
    if (!lvl0_ready(p, key0, bits, seed, b, 0, count)) return RTFHE_ERR_INVALID;
    return production(seed, [&](Rng& r) { return encrypt_tlwe(r, SeedMask{seed, 0}, p, key0, [&](size_t g) { return bit_word(bits[g]); }, b, count); });
}

int rtfhe_tlwe_encrypt_torus_seeded(const rtfhe_params* p, const int32_t* key0, const uint32_t* mu, uint32_t* seed, uint32_t* b, size_t count) {
    if (!lvl0_ready(p, key0, mu, seed, b, 0, count)) return RTFHE_ERR_INVALID;
    return production(seed, [&](Rng& r) { return encrypt_tlwe(r, SeedMask{seed, 0}, p, key0, [&](size_t g) { return mu[g]; }, b, count); });
}

int rtfhe_ksk_keygen_seeded(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* seed, uint32_t* b) {
    if (!ksk_ready(p, key0, key1, seed, b, 0)) return RTFHE_ERR_INVALID;
    return production_source(seed, [&](const Source& src) { return ksk_keygen(p, src, SeedMask{seed, 0}, key0, key1, b); });
}

// ---- TEST ONLY: the noise from a 64-bit seed (xoshiro256**, not a CSPRNG); the mask seed and its first row are the caller's ----
int rtfhe_trlwe_encrypt_torus_seeded_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                   const uint32_t* mu, uint32_t* b, size_t count) {
    if (!lvl1_ready(p, key1, mu, seed, b, first_row, count, 1)) return RTFHE_ERR_INVALID;
    return deterministic(noise_seed, [&](Rng& r) { return encrypt_trlwe(r, SeedMask{seed, first_row}, p, key1, mu, b, count); });
}

int rtfhe_trgsw_encrypt_bits_seeded_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                  const uint8_t* bits, uint32_t* b, size_t count) {
    if (!lvl1_ready(p, key1, bits, seed, b, first_row, count, trgsw_rows_each(p))) return RTFHE_ERR_INVALID;
    return deterministic(noise_seed, [&](Rng& r) { return encrypt_trgsw_bits(r, SeedMask{seed, first_row}, p, key1, bits, b, count); });
}

int rtfhe_trgsw_encrypt_polys_seeded_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                   const int32_t* mu, uint32_t* b, size_t count) {
    if (!lvl1_ready(p, key1, mu, seed, b, first_row, count, trgsw_rows_each(p))) return RTFHE_ERR_INVALID;
    return deterministic(noise_seed, [&](Rng& r) { return encrypt_trgsw_polys(r, SeedMask{seed, first_row}, p, key1, mu, b, count); });
}

int rtfhe_packing_keygen_seeded_deterministic(const rtfhe_params* p, uint64_t noise_seed, const int32_t* key0, const int32_t* key1, const uint32_t* seed,
                                              uint64_t first_row, uint32_t* b) {
    if (!packing_ready(p, key0, key1, seed, b, first_row)) return RTFHE_ERR_INVALID;
    return packing_keygen(p, Source::from_seed(noise_seed), SeedMask{seed, first_row}, key0, key1, b);
}

int rtfhe_tlwe_encrypt_bits_seeded_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                 const uint8_t* bits, uint32_t* b, size_t count) {
    if (!lvl0_ready(p, key0, bits, seed, b, first_row, count)) return RTFHE_ERR_INVALID;
    return deterministic(noise_seed, [&](Rng& r) { return encrypt_tlwe(r, SeedMask{seed, first_row}, p, key0, [&](size_t g) { return bit_word(bits[g]); }, b, count); });
}

int rtfhe_tlwe_encrypt_torus_seeded_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                  const uint32_t* mu, uint32_t* b, size_t count) {
    if (!lvl0_ready(p, key0, mu, seed, b, first_row, count)) return RTFHE_ERR_INVALID;
    return deterministic(noise_seed, [&](Rng& r) { return encrypt_tlwe(r, SeedMask{seed, first_row}, p, key0, [&](size_t g) { return mu[g]; }, b, count); });
}

int rtfhe_ksk_keygen_seeded_deterministic(const rtfhe_params* p, uint64_t noise_seed, const int32_t* key0, const int32_t* key1, const uint32_t* seed,
                                          uint64_t first_row, uint32_t* b) {
    if (!ksk_ready(p, key0, key1, seed, b, first_row)) return RTFHE_ERR_INVALID;
    return ksk_keygen(p, Source::from_seed(noise_seed), SeedMask{seed, first_row}, key0, key1, b);
}

}  // extern "C"
