// rtfhe_tlwe_seeded.cpp -- host only: seeded lvl0 ciphertexts and the seeded key-switching key (include/rtfhe.h, "seeded lvl0 ciphertexts").
// The mask rule for rows of length n on the CPU (rtfhe_tlwe_mask_expand, rtfhe_tlwe_seeded_expand: the oracle of k_tlwe_seeded_expand and the
// path of a server without this library's GPU side), the seeded lvl0 encryptors, the seeded key-switching key generation, and the argument checks
// of every seeded lvl0 call, device calls included (rtfhe_tlwe_seeded_plan.h).  No HIP call in this unit.
// Noise and message words are drawn as rtfhe_keygen.cpp's tlwe_encrypt draws them (rtfhe_sampling.hpp); only the mask differs: it is the ChaCha20
// keystream of the public seed, all 32 bits of every word, and never the generator the noise comes from.
#include "rtfhe_tlwe_seeded_plan.h"

#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "rtfhe_sampling.hpp"

namespace {

using namespace rtfhe_sampling;

int refuse(char* err, size_t err_len, const std::string& msg) {
    if (err && err_len) std::snprintf(err, err_len, "%s", msg.c_str());
    return RTFHE_ERR_INVALID;
}

// do rows first_row .. first_row + rows - 1 exist (first_row + rows <= 2^64)?
bool rows_ok(uint64_t first_row, size_t rows) { return first_row == 0 || (uint64_t)rows <= (uint64_t)0 - first_row; }

// the mask rule: row R is the keystream of stream R, blocks 0 .. ceil(n / 16) - 1, cut at n words
void mask_row(int n, const uint32_t* seed, uint64_t R, uint32_t* a) {
    int c = 0;
    for (; 16 * (c + 1) <= n; c++) rtfhe::chacha_block(seed, (uint64_t)c, R, a + 16 * c);
    if (16 * c < n) {
        uint32_t last[16];
        rtfhe::chacha_block(seed, (uint64_t)c, R, last);
        std::memcpy(a + 16 * c, last, (size_t)(n - 16 * c) * 4);
    }
}

bool binary(const int32_t* key, int n) {
    for (int i = 0; i < n; i++) if (key[i] != 0 && key[i] != 1) return false;
    return true;
}

const float ALPHA_KS = 1.0f / 32768.0f;      // 2^-15, tlwe.rs:176

// b = <a, key0> + e + msg with a = mask row R of the seed: rtfhe_keygen.cpp's tlwe_encrypt with the mask given instead of drawn
uint32_t masked_b(Rng& r, int n, const int32_t* key0, const uint32_t* seed, uint64_t R, uint32_t msg, uint32_t* a) {
    mask_row(n, seed, R, a);
    const uint32_t e = gaussian_torus(r, ALPHA_KS);
    uint32_t b = 0;
    for (int i = 0; i < n; i++) if (key0[i]) b += a[i];
    return b + e + msg;
}

template <typename Msg>
int encrypt(const rtfhe_params* p, Rng& r, const int32_t* key0, const uint32_t* seed, uint64_t first_row, Msg msg, uint32_t* b, size_t count) {
    std::vector<uint32_t> a((size_t)p->n);
    for (size_t g = 0; g < count; g++) b[g] = masked_b(r, p->n, key0, seed, first_row + g, msg(g), a.data());
    return 0;
}

size_t ksk_row_count(const rtfhe_params* p) { return (size_t)p->N * (size_t)p->ks_t * (((size_t)1 << p->ks_basebit) - 1); }

// rtfhe_keygen.cpp's key-switching key with the masks from the seed: row (i, lv, d) is mask row first_row + (i t + lv)(base - 1) + d; one noise
// generator per coefficient i, striped over the threads, from the same streams (secure: ChaCha domain 2) and seeds (deterministic)
int ksk_keygen(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, const uint32_t* seed, uint64_t first_row, uint32_t* b) {
    const int n = p->n, N = p->N, t = p->ks_t, bb = p->ks_basebit;
    const size_t base1 = ((size_t)1 << bb) - 1;
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
    uint64_t s_ks = 0;
    if (!src.secure) { Xoshiro root(src.seed); root.next(); s_ks = root.next(); }
    auto body = [&](Rng& r, int i, uint32_t* a) {
        for (int lv = 0; lv < t; lv++)
            for (size_t d = 0; d < base1; d++) {
                const size_t row = ((size_t)i * t + lv) * base1 + d;
                b[row] = masked_b(r, n, key0, seed, first_row + row, ks_digit_share(key1[i], bb, lv, (int)d), a);
            }
    };
    auto work = [&](int tid) {
        std::vector<uint32_t> a((size_t)n);
        for (int i = tid; i < N; i += nthreads) {
            if (src.secure) { ChaCha r(src.key, ((uint64_t)2 << 32) | (uint32_t)i); body(r, i, a.data()); }
            else { Xoshiro r(s_ks + 0xbf58476d1ce4e5b9ull * (uint64_t)(i + 1)); body(r, i, a.data()); }
        }
    };
    std::vector<std::thread> th;
    for (int k = 0; k < nthreads; k++) th.emplace_back(work, k);
    for (auto& x : th) x.join();
    return 0;
}

// what every seeded lvl0 encryptor asks first: a valid parameter set, a binary lvl0 key, rows that exist
bool encrypt_ready(const rtfhe_params* p, const int32_t* key0, const void* in, const uint32_t* seed, const void* b, uint64_t first_row, size_t count) {
    if (!valid(p) || !key0 || !in || !seed || !b) return false;
    return rows_ok(first_row, count) && binary(key0, p->n);
}

bool ksk_ready(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, const uint32_t* seed, const void* b, uint64_t first_row) {
    if (!valid(p) || !key0 || !key1 || !seed || !b) return false;
    return rows_ok(first_row, ksk_row_count(p)) && binary(key0, p->n) && binary(key1, p->N);
}

// the production forms' two draws from the OS: the public mask seed, and -- separately -- the key of the noise generator
bool fresh(uint32_t* seed, Source& noise) { return os_random(seed, 8 * sizeof(uint32_t)) && Source::from_os(noise); }

uint32_t bit_word(uint8_t bit) { return torus_from_f32(bit ? 0.125f : -0.125f); }

}  // namespace

extern "C" {

int rtfhe_tlwe_seeded_plan(int32_t what, int32_t n, const void* seed, uint64_t first_row, const void* b, const void* out, size_t rows, char* err,
                           size_t err_len) {
    if (err && err_len) err[0] = 0;
    const bool upload = what == RTFHE_TLWE_SEEDED_UPLOAD, host = what == RTFHE_TLWE_SEEDED_HOST;
    if (!seed || !b || (!upload && !out)) return refuse(err, err_len, "null argument");
    if (n < 1 || (!host && n > 767)) return refuse(err, err_len, "n = " + std::to_string(n) + (host ? " is below 1" : " is outside [1, 767]"));
    if (rows < 1) return refuse(err, err_len, "rows = 0: a seeded lvl0 object has at least one row");
    if (!rows_ok(first_row, rows))
        return refuse(err, err_len, "rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " + std::to_string(rows) + ") pass 2^64");
    const size_t w = (size_t)n + 1, nb = ((size_t)n + 15) / 16;
    if (!host && rows > (size_t)0x7fffffff / nb) return refuse(err, err_len, "rows * ceil(n / 16) too large (it must be below 2^31)");
    if (host && rows > ((size_t)-1 / 4) / w) return refuse(err, err_len, "rows * (n + 1) words too large");
    if (upload) return 0;
    const uintptr_t i0 = (uintptr_t)b, o0 = (uintptr_t)out;
    if (what == RTFHE_TLWE_SEEDED_DEVICE && ((i0 | o0) & 3)) return refuse(err, err_len, "d_b and d_out must be 4-byte aligned");
    const size_t in_bytes = rows * 4, out_bytes = rows * w * 4;
    if (i0 < o0 + out_bytes && o0 < i0 + in_bytes) return refuse(err, err_len, "the output overlaps the b words");
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
int rtfhe_tlwe_encrypt_bits_seeded(const rtfhe_params* p, const int32_t* key0, const uint8_t* bits, uint32_t* seed, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key0, bits, seed, b, 0, count)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);
    return encrypt(p, r, key0, seed, 0, [&](size_t g) { return bit_word(bits[g]); }, b, count);
}

int rtfhe_tlwe_encrypt_torus_seeded(const rtfhe_params* p, const int32_t* key0, const uint32_t* mu, uint32_t* seed, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key0, mu, seed, b, 0, count)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);
    return encrypt(p, r, key0, seed, 0, [&](size_t g) { return mu[g]; }, b, count);
}

int rtfhe_ksk_keygen_seeded(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* seed, uint32_t* b) {
    if (!ksk_ready(p, key0, key1, seed, b, 0)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    return ksk_keygen(p, src, key0, key1, seed, 0, b);
}

// ---- TEST ONLY: the noise from a 64-bit seed (xoshiro256**, not a CSPRNG); the mask seed and its first row are the caller's ----
int rtfhe_tlwe_encrypt_bits_seeded_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                 const uint8_t* bits, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key0, bits, seed, b, first_row, count)) return RTFHE_ERR_INVALID;
    Xoshiro r(noise_seed);
    return encrypt(p, r, key0, seed, first_row, [&](size_t g) { return bit_word(bits[g]); }, b, count);
}

int rtfhe_tlwe_encrypt_torus_seeded_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                  const uint32_t* mu, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key0, mu, seed, b, first_row, count)) return RTFHE_ERR_INVALID;
    Xoshiro r(noise_seed);
    return encrypt(p, r, key0, seed, first_row, [&](size_t g) { return mu[g]; }, b, count);
}

int rtfhe_ksk_keygen_seeded_deterministic(const rtfhe_params* p, uint64_t noise_seed, const int32_t* key0, const int32_t* key1, const uint32_t* seed,
                                          uint64_t first_row, uint32_t* b) {
    if (!ksk_ready(p, key0, key1, seed, b, first_row)) return RTFHE_ERR_INVALID;
    return ksk_keygen(p, Source::from_seed(noise_seed), key0, key1, seed, first_row, b);
}

}  // extern "C"
