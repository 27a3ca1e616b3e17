// rtfhe_encrypt.hpp -- host only: the one encryptor core behind every client-side encryptor, unseeded (rtfhe_keygen.cpp) and seeded
// (rtfhe_seeded.cpp) alike.  A ciphertext row is mask, then noise, then the inner / negacyclic product with the binary key, then the message; the
// two families differ in one thing, where the mask comes from, and that is a type (DrawnMask, SeedMask) handed to the same code.  So a seeded
// object's noise and message words are drawn by the very statements that draw its unseeded twin's.  Follows:
//   TLWE encrypt               hom_nand/src/tlwe.rs:181-241
//   TRLWE zero encryption      hom_nand/src/trlwe.rs:127-137
//   TRGSW encryption of a bit  hom_nand/src/trgsw.rs:118-138,217-229
//   KeySwitchingKey::new       hom_nand/src/tlwe.rs:247-277
// The generators and the samplers: rtfhe_sampling.hpp.
#pragma once

#include <thread>
#include <vector>

#include "rtfhe_sampling.hpp"

namespace rtfhe_encrypt {

using namespace rtfhe_sampling;

const float ALPHA_KS = 1.0f / 32768.0f;      // 2^-15, tlwe.rs:176: lvl0 ciphertexts and the key-switching key
const float ALPHA_BK = 1.0f / 33554432.0f;   // 2^-25, trlwe.rs:77: everything under the lvl1 key

inline bool binary(const int32_t* key, int n) {
    for (int i = 0; i < n; i++) if (key[i] != 0 && key[i] != 1) return false;
    return true;
}

// do rows first_row .. first_row + rows - 1 exist (first_row + rows <= 2^64)?
inline bool rows_ok(uint64_t first_row, size_t rows) { return first_row == 0 || (uint64_t)rows <= (uint64_t)0 - first_row; }

// the mask rule: row R of a public seed is the ChaCha20 keystream of stream R, blocks 0 .. ceil(len / 16) - 1, cut at len words (ring rows:
// len = N, a multiple of 16; lvl0 rows: len = n, any)
inline void mask_row(int len, const uint32_t* seed, uint64_t R, uint32_t* a) {
    int c = 0;
    for (; 16 * (c + 1) <= len; c++) rtfhe::chacha_block(seed, (uint64_t)c, R, a + 16 * c);
    if (16 * c < len) {
        uint32_t last[16];
        rtfhe::chacha_block(seed, (uint64_t)c, R, last);
        std::memcpy(a + 16 * c, last, (size_t)(len - 16 * c) * 4);
    }
}

// ---- mask sources.  row(r, R, len, a) fills the mask of row R; `kept` says whether the mask words are part of the ciphertext's stored form ----
// drawn from the generator the noise comes from, one word at a time and before the noise; stored with the ciphertext
struct DrawnMask {
    static constexpr bool kept = true;
    void row(Rng& r, uint64_t, int len, uint32_t* a) const { for (int i = 0; i < len; i++) a[i] = uniform_torus(r); }
};
// row first_row + R of a public seed, all 32 bits of every word and never the generator the noise comes from; only the b halves are stored
struct SeedMask {
    static constexpr bool kept = false;
    const uint32_t* seed; uint64_t first_row;
    void row(Rng&, uint64_t R, int len, uint32_t* a) const { mask_row(len, seed, first_row + R, a); }
};

// ---- rows ----
// b = <a, key> + e + msg.  Any non-zero key word counts as 1: the unseeded lvl0 entry points do not check that key0 is binary.
template <class Mask>
uint32_t tlwe_encrypt(Rng& r, const Mask& mask, uint64_t R, int n, const int32_t* key, uint32_t msg, uint32_t* a) {
    mask.row(r, R, n, a);
    const uint32_t e = gaussian_torus(r, ALPHA_KS);
    uint32_t b = 0;
    for (int i = 0; i < n; i++) if (key[i]) b += a[i];
    return b + e + msg;
}

// b = a * s + e under the mask given (exact negacyclic product with the binary key; the reference uses its FFT here)
// (centred: the noise from gaussian_torus_centred, for the packing key)
inline void trlwe_zero_under(Rng& r, int N, const int32_t* key, bool centred, const uint32_t* a, uint32_t* b) {
    for (int k = 0; k < N; k++) b[k] = centred ? gaussian_torus_centred(r, (double)ALPHA_BK) : gaussian_torus(r, ALPHA_BK);
    for (int j = 0; j < N; j++) {
        if (!key[j]) continue;
        for (int k = 0; k < N - j; k++) b[k + j] += a[k];
        for (int k = N - j; k < N; k++) b[k + j - N] -= a[k];
    }
}

template <class Mask>
void trlwe_zero(Rng& r, const Mask& mask, uint64_t R, int N, const int32_t* key, bool centred, uint32_t* b, uint32_t* a) {
    mask.row(r, R, N, a);
    trlwe_zero_under(r, N, key, centred, a, b);
}

// where row R of a stored object lies: (b, a) of an lvl0 row (DrawnMask: [n + 1], a then b; SeedMask: the b word, a in scratch) ...
template <class Mask>
void tlwe_row(Rng& r, const Mask& mask, uint64_t R, int n, const int32_t* key, uint32_t msg, uint32_t* out, uint32_t* scratch) {
    uint32_t* row = out + R * (Mask::kept ? (size_t)n + 1 : 1);
    row[Mask::kept ? n : 0] = tlwe_encrypt(r, mask, R, n, key, msg, Mask::kept ? row : scratch);
}
// ... and of a ring row (DrawnMask: [2][N], b then a; SeedMask: [N], a in scratch); returns b, for the message to be added
template <class Mask>
uint32_t* trlwe_row(Rng& r, const Mask& mask, uint64_t R, int N, const int32_t* key, bool centred, uint32_t* out, uint32_t* scratch) {
    uint32_t* b = out + R * (Mask::kept ? 2 : 1) * (size_t)N;
    trlwe_zero(r, mask, R, N, key, centred, b, Mask::kept ? b + N : scratch);
    return b;
}

// One TRGSW sample under key1 (trgsw.rs:118-138, 217-229): 2l TRLWE encryptions of zero plus the message times the gadget, share(k, c) = the
// message word of gadget position k at coefficient c, on row k's b polynomial and on row l + k's a polynomial.  Masks: rows row0 .. row0 + 2l - 1.
// DrawnMask: ct [2][2l][N], comp 0 = the b polynomials (TRGSWRep.cipher), comp 1 = the a polynomials (p_key); SeedMask: ct [2l][N], the b's.
// Rows k < l carry the share on b.  Rows l + k carry it on the a polynomial, which in the seeded form must stay the seed's keystream: the zero
// encryption is made under a - share, a uniform polynomial as well, so that the expanded row (b, a) is the unseeded encryptor's
// (b, (a - share) + share) word for word in form and in distribution (its phase: e - share * s).  The drawn form stores (b, a + share).
template <class Mask, class Share>
void trgsw_rows(Rng& r, const Mask& mask, uint64_t row0, const rtfhe_params* p, const int32_t* key1, Share share, uint32_t* ct, uint32_t* scratch) {
    const int N = p->N, l = p->l;
    for (int j = 0; j < 2 * l; j++) {
        uint32_t* b = ct + (size_t)j * N;
        uint32_t* a = Mask::kept ? ct + ((size_t)2 * l + j) * N : scratch;
        mask.row(r, row0 + (uint64_t)j, N, a);
        if (!Mask::kept && j >= l) for (int c = 0; c < N; c++) a[c] -= share(j - l, c);
        trlwe_zero_under(r, N, key1, false, a, b);
        if (j < l) for (int c = 0; c < N; c++) b[c] += share(j, c);
        else if (Mask::kept) for (int c = 0; c < N; c++) a[c] += share(j - l, c);
    }
}

// ---- encryptors of count rows / samples, numbered from 0 (a SeedMask adds its first_row) ----
// lvl0 ciphertexts of the torus words msg(g)
template <class Mask, class Msg>
int encrypt_tlwe(Rng& r, const Mask& mask, const rtfhe_params* p, const int32_t* key0, Msg msg, uint32_t* out, size_t count) {
    std::vector<uint32_t> scratch(Mask::kept ? 0 : (size_t)p->n);
    for (size_t g = 0; g < count; g++) tlwe_row(r, mask, g, p->n, key0, msg(g), out, scratch.data());
    return 0;
}
inline uint32_t bit_word(uint8_t bit) { return torus_from_f32(bit ? 0.125f : -0.125f); }

// TRLWE encryptions of the polynomials mu[count][N] under key1 (encrypted tables): a zero encryption as the bootstrapping key's rows, b += mu
template <class Mask>
int encrypt_trlwe(Rng& r, const Mask& mask, const rtfhe_params* p, const int32_t* key1, const uint32_t* mu, uint32_t* out, size_t count) {
    const int N = p->N;
    std::vector<uint32_t> scratch(Mask::kept ? 0 : (size_t)N);
    for (size_t g = 0; g < count; g++) {
        uint32_t* b = trlwe_row(r, mask, g, N, key1, false, out, scratch.data());
        for (int k = 0; k < N; k++) b[k] += mu[g * (size_t)N + k];
    }
    return 0;
}

// TRGSW samples of share_of(g)(k, c), 2l mask rows each
template <class Mask, class ShareOf>
int encrypt_trgsw(Rng& r, const Mask& mask, const rtfhe_params* p, const int32_t* key1, ShareOf share_of, uint32_t* out, size_t count) {
    const size_t rows = (size_t)2 * p->l, words = (Mask::kept ? 2 : 1) * rows * (size_t)p->N;
    std::vector<uint32_t> scratch(Mask::kept ? 0 : (size_t)p->N);
    for (size_t g = 0; g < count; g++) trgsw_rows(r, mask, g * rows, p, key1, share_of(g), out + g * words, scratch.data());
    return 0;
}
// of a bit: mu / Bg^(k+1) on the constant coefficient (an entry of the bootstrapping key and a caller's selector alike)
struct BitShare {
    uint32_t t2[32];
    BitShare(const rtfhe_params* p, int32_t mu) { for (int k = 0; k < p->l; k++) t2[k] = trgsw_bit_share(mu, p->bgbit, k); }
    uint32_t operator()(int k, int c) const { return c == 0 ? t2[k] : 0u; }
};
// of the small-integer polynomial mu(X): the integer mu_c * 2^(32 - (k+1) bgbit), wrapping (>= 0 shifts: valid(p) holds l * bgbit <= 32), over
// all N coefficients where BitShare adds to coefficient 0 -- the same 2l zero encryptions, drawn in the same order, so that a constant
// polynomial mu = bit gives BitShare's words.  An encrypted weight row of a linear layer (rtfhe_trlwe_mul_trgsw_batch).
struct PolyShare {
    const int32_t* mu; int bgbit;
    uint32_t operator()(int k, int c) const { return (uint32_t)mu[c] << (32 - (k + 1) * bgbit); }
};
template <class Mask>
int encrypt_trgsw_bits(Rng& r, const Mask& mask, const rtfhe_params* p, const int32_t* key1, const uint8_t* bits, uint32_t* out, size_t count) {
    return encrypt_trgsw(r, mask, p, key1, [&](size_t g) { return BitShare(p, bits[g] ? 1 : 0); }, out, count);
}
template <class Mask>
int encrypt_trgsw_polys(Rng& r, const Mask& mask, const rtfhe_params* p, const int32_t* key1, const int32_t* mu, uint32_t* out, size_t count) {
    return encrypt_trgsw(r, mask, p, key1, [&](size_t g) { return PolyShare{mu + g * (size_t)p->N, p->bgbit}; }, out, count);
}

// ---- keys: one generator per coefficient ----
// The generator of coefficient i.  Secure: the ChaCha stream (domain, i) under the OS key.  Deterministic: xoshiro seeded base + mult * (i + 1),
// the seeds of round 1 (fixtures stay valid).
template <class Body>
void coefficient_rng(const Source& src, int domain, uint64_t base, uint64_t mult, int i, Body body) {
    if (src.secure) { ChaCha r(src.key, ((uint64_t)domain << 32) | (uint32_t)i); body(r); }
    else { Xoshiro r(base + mult * (uint64_t)(i + 1)); body(r); }
}
// the k-th word (from 1) of the deterministic source's root generator: the base seed of the bootstrapping key (1), the key-switching key (2)
// and the packing key (3)
inline uint64_t root_word(const Source& src, int k) {
    if (src.secure) return 0;
    Xoshiro root(src.seed);
    uint64_t v = 0;
    for (int j = 0; j < k; j++) v = root.next();
    return v;
}
// body(r, i) for i = 0 .. count - 1, each under its own generator, striped over at most 16 threads: the words do not depend on the thread count
template <class Body>
void striped(const Source& src, int domain, uint64_t base, uint64_t mult, int count, Body body) {
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
    auto work = [&](int t) {
        for (int i = t; i < count; i += nthreads) coefficient_rng(src, domain, base, mult, i, [&](Rng& r) { body(r, i); });
    };
    std::vector<std::thread> th;
    for (int t = 0; t < nthreads; t++) th.emplace_back(work, t);
    for (auto& x : th) x.join();
}

inline size_t digit_row_count(const rtfhe_params* p) { return (size_t)p->ks_t * (((size_t)1 << p->ks_basebit) - 1); }
// A key-switch-shaped key of the bits[count]: rows (i, lv, d), lv < t, d < base - 1, in this order, row(r, R, msg, scratch) with
// R = (i t + lv)(base - 1) + d and msg = (d + 1) bits[i] / 2^(basebit (lv + 1)); scratch: scratch_len words of the thread's own.
template <class Row>
void digit_rows(const rtfhe_params* p, const Source& src, int domain, uint64_t base, uint64_t mult, const int32_t* bits, int count, size_t scratch_len,
                Row row) {
    const size_t base1 = ((size_t)1 << p->ks_basebit) - 1;
    striped(src, domain, base, mult, count, [&](Rng& r, int i) {
        std::vector<uint32_t> scratch(scratch_len);
        for (int lv = 0; lv < p->ks_t; lv++)
            for (size_t d = 0; d < base1; d++)
                row(r, ((size_t)i * p->ks_t + lv) * base1 + d, ks_digit_share(bits[i], p->ks_basebit, lv, (int)d), scratch.data());
    });
}

// The key-switching key (KeySwitchingKey::new without its last entry per level): row (i, lv, d) an lvl0 encryption under key0 of the digit share
// of key1[i].  Secure: ChaCha streams of domain 2.
template <class Mask>
int ksk_keygen(const rtfhe_params* p, const Source& src, const Mask& mask, const int32_t* key0, const int32_t* key1, uint32_t* out) {
    digit_rows(p, src, 2, root_word(src, 2), 0xbf58476d1ce4e5b9ull, key1, p->N, Mask::kept ? 0 : (size_t)p->n,
               [&](Rng& r, size_t R, uint32_t msg, uint32_t* scratch) { tlwe_row(r, mask, R, p->n, key0, msg, out, scratch); });
    return 0;
}

// The packing key (rtfhe_packing_keygen; include/rtfhe.h): row (i, lv, d) a TRLWE under key1 of the constant polynomial digit share of key0[i]
// (zero-mean noise: gaussian_torus_centred).  Secure: ChaCha streams of domain 4.  ks parameters other than (8, 2) are refused by the entry points:
// the one instantiation the packing key switch has.
template <class Mask>
int packing_keygen(const rtfhe_params* p, const Source& src, const Mask& mask, const int32_t* key0, const int32_t* key1, uint32_t* out) {
    digit_rows(p, src, 4, root_word(src, 3), 0xd6e8feb86659fd93ull, key0, p->n, Mask::kept ? 0 : (size_t)p->N,
               [&](Rng& r, size_t R, uint32_t msg, uint32_t* scratch) { trlwe_row(r, mask, R, p->N, key1, true, out, scratch)[0] += msg; });
    return 0;
}

// ---- the entry points' scaffolds: a refused argument is RTFHE_ERR_INVALID (the entry point's own check, before anything is drawn), an OS that
// gives no randomness RTFHE_ERR_STATE ----
// the production forms' draws from the OS: the public mask seed of a seeded object (none: null), and -- separately -- the key of the noise generator
inline bool fresh(uint32_t* mask_seed, Source& noise) { return (!mask_seed || os_random(mask_seed, 8 * sizeof(uint32_t))) && Source::from_os(noise); }

// production: body(src) under a fresh OS key ...
template <class Body>
int production_source(uint32_t* mask_seed, Body body) {
    Source src;
    if (!fresh(mask_seed, src)) return RTFHE_ERR_STATE;
    return body(src);
}
// ... or body(r) with r its stream 0: a fresh OS key per call, mask and noise are never reused
template <class Body>
int production(uint32_t* mask_seed, Body body) {
    return production_source(mask_seed, [&](const Source& src) { ChaCha r(src.key, 0); return body(r); });
}
// TEST ONLY: body(r) with r reproducible from a 64-bit seed (xoshiro256**, not a CSPRNG)
template <class Body>
int deterministic(uint64_t seed, Body body) {
    Xoshiro r(seed);
    return body(r);
}

}  // namespace rtfhe_encrypt
