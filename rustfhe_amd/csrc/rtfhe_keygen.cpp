// rtfhe_keygen.cpp -- host-side key generation and TLWE encryption/decryption behind the C ABI.
// Off the timed path (the reference's TFHE::new is setup too, hom_nand/src/tfhe.rs:21-25), kept on the
// host like the reference's.  Follows:
//   TLWE encrypt/decrypt       hom_nand/src/tlwe.rs:181-241
//   TRLWE zero encryption      hom_nand/src/trlwe.rs:127-137 (also of encrypted tables: rtfhe_trlwe_encrypt_torus)
//   TRGSW encryption of a bit  hom_nand/src/trgsw.rs:118-138,217-229
//   BootstrappingKey::new      hom_nand/src/tfhe.rs:119-126 (torus form; the device transforms it)
//   KeySwitchingKey::new       hom_nand/src/tlwe.rs:247-277
//   torus!(f32)                utils/src/math.rs:691-696
// Randomness, the generators and the torus samplers: rtfhe_sampling.hpp (shared with the seeded encryptors of rtfhe_seeded.cpp); the ChaCha20
// block function: rtfhe_chacha.hpp.
#include "../../include/rtfhe.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "rtfhe_sampling.hpp"

namespace {

using namespace rtfhe_sampling;

void tlwe_encrypt(Rng& r, int n, const int32_t* key, uint32_t msg, float alpha, uint32_t* ct) {
    uint32_t b = 0;
    for (int i = 0; i < n; i++) ct[i] = uniform_torus(r);
    const uint32_t e = gaussian_torus(r, alpha);
    for (int i = 0; i < n; i++) if (key[i]) b += ct[i];
    ct[n] = b + e + msg;
}

// b = a * s + e  (exact negacyclic product with the binary key; the reference uses its FFT here)
// (centred: the noise from gaussian_torus_centred, for the packing key)
void trlwe_zero(Rng& r, int N, const int32_t* key, float alpha, uint32_t* b, uint32_t* a, bool centred = false) {
    for (int k = 0; k < N; k++) a[k] = uniform_torus(r);
    for (int k = 0; k < N; k++) b[k] = centred ? gaussian_torus_centred(r, (double)alpha) : gaussian_torus(r, alpha);
    for (int j = 0; j < N; j++) {
        if (!key[j]) continue;
        for (int k = 0; k < N - j; k++) b[k + j] += a[k];
        for (int k = N - j; k < N; k++) b[k + j - N] -= a[k];
    }
}

// TRGSW encryption of the bit mu under key1 (trgsw.rs:118-138, 217-229): 2l TRLWE encryptions of zero (alpha = 2^-25, trlwe.rs:77) plus mu
// times the gadget, mu / Bg^(k+1) on the constant coefficient of row k's b polynomial and of row l + k's a polynomial.  ct: [2][2l][N], comp 0 =
// the b polynomials (TRGSWRep.cipher), comp 1 = the a polynomials (p_key).  An entry of the bootstrapping key and a caller's selector alike.
void trgsw_encrypt(Rng& r, const rtfhe_params* p, const int32_t* key1, int32_t mu, uint32_t* ct) {
    const int N = p->N, l = p->l, rows = 2 * l;
    const float alpha_bk = 1.0f / 33554432.0f;   // 2^-25, trlwe.rs:77
    for (int j = 0; j < rows; j++) trlwe_zero(r, N, key1, alpha_bk, ct + (size_t)j * N, ct + ((size_t)rows + j) * N);
    for (int k = 0; k < l; k++) {
        const uint32_t t2 = trgsw_bit_share(mu, p->bgbit, k);
        ct[(size_t)k * N] += t2;
        ct[((size_t)rows + k + l) * N] += t2;
    }
}

// TRGSW encryption of the small-integer polynomial mu(X) under key1: trgsw_encrypt with mu(X) / Bg^(k+1) over all N coefficients where that adds
// the bit's share to coefficient 0 (the same 2l zero encryptions, drawn in the same order, so that a constant polynomial mu = bit gives
// trgsw_encrypt's words).  The share is the integer mu_c * 2^(32 - (k+1) bgbit), wrapping: an encrypted weight row of a linear layer
// (rtfhe_trlwe_mul_trgsw_batch), where trgsw_encrypt's are a selector's bit.
void trgsw_encrypt_poly(Rng& r, const rtfhe_params* p, const int32_t* key1, const int32_t* mu, uint32_t* ct) {
    const int N = p->N, l = p->l, rows = 2 * l;
    const float alpha_bk = 1.0f / 33554432.0f;   // 2^-25, trlwe.rs:77
    for (int j = 0; j < rows; j++) trlwe_zero(r, N, key1, alpha_bk, ct + (size_t)j * N, ct + ((size_t)rows + j) * N);
    for (int k = 0; k < l; k++) {
        const int sh = 32 - (k + 1) * p->bgbit;      // >= 0: valid(p) holds l * bgbit <= 32
        uint32_t* b = ct + (size_t)k * N;
        uint32_t* a = ct + ((size_t)rows + k + l) * N;
        for (int c = 0; c < N; c++) {
            const uint32_t t2 = (uint32_t)mu[c] << sh;
            b[c] += t2;
            a[c] += t2;
        }
    }
}

// key material for given secret keys (TFHE::new, hom_nand/src/tfhe.rs:21-25); one generator per TRGSW / per KSK coefficient
int keygen_material(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    const int n = p->n, N = p->N, l = p->l, rows = 2 * l;
    for (int i = 0; i < n; i++) if (key0[i] != 0 && key0[i] != 1) return RTFHE_ERR_INVALID;
    for (int i = 0; i < N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    const float alpha_ks = 1.0f / 32768.0f;      // 2^-15, tlwe.rs:176
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
    uint64_t s_bk = 0, s_ks = 0;
    if (!src.secure) { Xoshiro root(src.seed); s_bk = root.next(); s_ks = root.next(); }
    // deterministic: the seeds of round 1 (fixtures stay valid); secure: ChaCha streams (domain, index) under the OS key
    auto row_rng = [&](int domain, int i, auto&& body) {
        if (src.secure) { ChaCha r(src.key, ((uint64_t)domain << 32) | (uint32_t)i); body(r); }
        else { Xoshiro r(domain == 1 ? s_bk + 0x9e3779b97f4a7c15ull * (uint64_t)(i + 1) : s_ks + 0xbf58476d1ce4e5b9ull * (uint64_t)(i + 1)); body(r); }
    };
    if (bk) {
        const size_t trgsw = (size_t)2 * rows * N;
        auto work = [&](int t) {
            for (int i = t; i < n; i += nthreads)
                row_rng(1, i, [&](Rng& r) { trgsw_encrypt(r, p, key1, key0[i], bk + (size_t)i * trgsw); });
        };
        std::vector<std::thread> th;
        for (int t = 0; t < nthreads; t++) th.emplace_back(work, t);
        for (auto& x : th) x.join();
    }
    if (ksk) {
        const int t = p->ks_t, bb = p->ks_basebit, base1 = (1 << bb) - 1;
        auto work = [&](int tid) {
            for (int i = tid; i < N; i += nthreads)
                row_rng(2, i, [&](Rng& r) {
                    for (int lv = 0; lv < t; lv++)
                        for (int d = 0; d < base1; d++) {
                            float pw = 1.0f;
                            for (int e = 0; e < bb * (lv + 1); e++) pw *= 0.5f;
                            const uint32_t item = torus_from_f32((float)key1[i] * pw * (float)(d + 1));
                            tlwe_encrypt(r, n, key0, item, alpha_ks, ksk + (((size_t)i * t + lv) * base1 + d) * (size_t)(n + 1));
                        }
                });
        };
        std::vector<std::thread> th;
        for (int k = 0; k < nthreads; k++) th.emplace_back(work, k);
        for (auto& x : th) x.join();
    }
    return 0;
}

// The packing key (rtfhe_packing_keygen; include/rtfhe.h): row (i, j, d) is a TRLWE under key1 of the constant polynomial
// (d + 1) key0[i] / 2^(basebit (j + 1)) with alpha = 2^-25 (zero-mean: gaussian_torus_centred), the message word formed as the key-switching
// key's above.  One generator per
// coefficient i, striped over the threads as keygen_material does; secure: ChaCha streams of domain 4, deterministic: seeds of its own.
int packing_keygen(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, uint32_t* pk) {
    const int n = p->n, N = p->N, t = p->ks_t, bb = p->ks_basebit, base1 = (1 << bb) - 1;
    if (t != 8 || bb != 2) return RTFHE_ERR_INVALID;      // the one instantiation the packing key switch has
    for (int i = 0; i < n; i++) if (key0[i] != 0 && key0[i] != 1) return RTFHE_ERR_INVALID;
    for (int i = 0; i < N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    const float alpha = 1.0f / 33554432.0f;      // 2^-25, trlwe.rs:77
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
    uint64_t s_pk = 0;
    if (!src.secure) { Xoshiro root(src.seed); root.next(); root.next(); s_pk = root.next(); }      // (the first two are keygen_material's)
    auto body = [&](Rng& r, int i) {
        for (int lv = 0; lv < t; lv++)
            for (int d = 0; d < base1; d++) {
                uint32_t* b = pk + (((size_t)i * t + lv) * base1 + d) * 2 * (size_t)N;
                trlwe_zero(r, N, key1, alpha, b, b + N, true);
                b[0] += ks_digit_share(key0[i], bb, lv, d);
            }
    };
    auto work = [&](int tid) {
        for (int i = tid; i < n; i += nthreads) {
            if (src.secure) { ChaCha r(src.key, ((uint64_t)4 << 32) | (uint32_t)i); body(r, i); }
            else { Xoshiro r(s_pk + 0xd6e8feb86659fd93ull * (uint64_t)(i + 1)); body(r, i); }
        }
    };
    std::vector<std::thread> th;
    for (int k = 0; k < nthreads; k++) th.emplace_back(work, k);
    for (auto& x : th) x.join();
    return 0;
}

// The reference's container shape from the compact one: [N][t][base][n+1] with entries 0 .. base-2 of every level copied and entry
// base-1 = TLWE(base * s_i / 2^(basebit (l+1))) freshly encrypted, as KeySwitchingKey::new fills it (hom_nand/src/tlwe.rs:252-274).
int ksk_expand_ref(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, const uint32_t* ksk, uint32_t* ksk_ref) {
    const int n = p->n, N = p->N, t = p->ks_t, bb = p->ks_basebit, base = 1 << bb;
    for (int i = 0; i < n; i++) if (key0[i] != 0 && key0[i] != 1) return RTFHE_ERR_INVALID;
    for (int i = 0; i < N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    const size_t w = (size_t)n + 1;
    const float alpha_ks = 1.0f / 32768.0f;
    for (int i = 0; i < N; i++) {
        auto body = [&](Rng& r) {
            for (int lv = 0; lv < t; lv++) {
                const size_t il = (size_t)i * t + lv;
                std::memcpy(ksk_ref + il * base * w, ksk + il * (base - 1) * w, (size_t)(base - 1) * w * sizeof(uint32_t));
                float pw = 1.0f;
                for (int e = 0; e < bb * (lv + 1); e++) pw *= 0.5f;
                const uint32_t item = torus_from_f32((float)key1[i] * pw * (float)base);
                tlwe_encrypt(r, n, key0, item, alpha_ks, ksk_ref + (il * base + (base - 1)) * w);
            }
        };
        if (src.secure) { ChaCha r(src.key, ((uint64_t)3 << 32) | (uint32_t)i); body(r); }
        else { Xoshiro r(src.seed + 0x94d049bb133111ebull * (uint64_t)(i + 1)); body(r); }
    }
    return 0;
}

int encrypt_bits(const rtfhe_params* p, Rng& r, const int32_t* key0, const uint8_t* bits, uint32_t* out, size_t count) {
    for (size_t g = 0; g < count; g++)
        tlwe_encrypt(r, p->n, key0, torus_from_f32(bits[g] ? 0.125f : -0.125f), 1.0f / 32768.0f, out + g * ((size_t)p->n + 1));
    return 0;
}

// the same with the plaintext torus words given directly (multi-bit messages for the programmable bootstrap)
int encrypt_torus(const rtfhe_params* p, Rng& r, const int32_t* key0, const uint32_t* mu, uint32_t* out, size_t count) {
    for (size_t g = 0; g < count; g++) tlwe_encrypt(r, p->n, key0, mu[g], 1.0f / 32768.0f, out + g * ((size_t)p->n + 1));
    return 0;
}

// TRLWE encryptions of the polynomials mu[count][N] under key1 (encrypted tables, rtfhe_lut_create_encrypted): trlwe_zero's
// b = a * s + e with alpha = 2^-25, as the bootstrapping key's rows, then b += mu.  Layout [count][2][N]: b then a.
int encrypt_trlwe(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint32_t* mu, uint32_t* out, size_t count) {
    const int N = p->N;
    for (int i = 0; i < N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    const float alpha = 1.0f / 33554432.0f;      // 2^-25, trlwe.rs:77
    for (size_t g = 0; g < count; g++) {
        uint32_t* b = out + g * 2 * (size_t)N;
        trlwe_zero(r, N, key1, alpha, b, b + N);
        for (int k = 0; k < N; k++) b[k] += mu[g * (size_t)N + k];
    }
    return 0;
}

// TRGSW encryptions of bits[count] under key1 (the selectors of a CMUX tree, rtfhe_trgsw_create): what keygen_material does per key bit
int encrypt_trgsw_bits(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint8_t* bits, uint32_t* out, size_t count) {
    for (int i = 0; i < p->N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    const size_t trgsw = (size_t)2 * 2 * p->l * p->N;
    for (size_t g = 0; g < count; g++) trgsw_encrypt(r, p, key1, bits[g] ? 1 : 0, out + g * trgsw);
    return 0;
}

// ... and of the integer polynomials mu[count][N] (encrypted weights, rtfhe_trlwe_mul_trgsw_batch)
int encrypt_trgsw_polys(const rtfhe_params* p, Rng& r, const int32_t* key1, const int32_t* mu, uint32_t* out, size_t count) {
    for (int i = 0; i < p->N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    const size_t trgsw = (size_t)2 * 2 * p->l * p->N;
    for (size_t g = 0; g < count; g++) trgsw_encrypt_poly(r, p, key1, mu + g * (size_t)p->N, out + g * trgsw);
    return 0;
}

}  // namespace

extern "C" {

// ---- production: OS CSPRNG ----
int rtfhe_keygen(const rtfhe_params* p, int32_t* key0, int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    {
        ChaCha r(src.key, 0);
        for (int i = 0; i < p->n; i++) key0[i] = (int32_t)(r.next() >> 63);
        for (int i = 0; i < p->N; i++) key1[i] = (int32_t)(r.next() >> 63);
    }
    return keygen_material(p, src, key0, key1, bk, ksk);
}

int rtfhe_keygen_with_keys(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    return keygen_material(p, src, key0, key1, bk, ksk);
}

int rtfhe_tlwe_encrypt_bits(const rtfhe_params* p, const int32_t* key0, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !bits || !out) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);          // a fresh OS key per call: mask and noise are never reused
    return encrypt_bits(p, r, key0, bits, out, count);
}

int rtfhe_tlwe_encrypt_torus(const rtfhe_params* p, const int32_t* key0, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !mu || !out) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);
    return encrypt_torus(p, r, key0, mu, out, count);
}

int rtfhe_trlwe_encrypt_torus(const rtfhe_params* p, const int32_t* key1, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);          // a fresh OS key per call
    return encrypt_trlwe(p, r, key1, mu, out, count);
}

int rtfhe_trgsw_encrypt_bits(const rtfhe_params* p, const int32_t* key1, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !bits || !out) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);          // a fresh OS key per call
    return encrypt_trgsw_bits(p, r, key1, bits, out, count);
}

int rtfhe_trgsw_encrypt_polys(const rtfhe_params* p, const int32_t* key1, const int32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);          // a fresh OS key per call
    return encrypt_trgsw_polys(p, r, key1, mu, out, count);
}

int rtfhe_ksk_expand_ref(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, const uint32_t* ksk, uint32_t* ksk_ref) {
    if (!valid(p) || !key0 || !key1 || !ksk || !ksk_ref) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    return ksk_expand_ref(p, src, key0, key1, ksk, ksk_ref);
}

int rtfhe_packing_keygen(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* pk) {
    if (!valid(p) || !key0 || !key1 || !pk) return RTFHE_ERR_INVALID;
    Source src;
    if (!Source::from_os(src)) return RTFHE_ERR_STATE;
    return packing_keygen(p, src, key0, key1, pk);
}

// ---- TEST ONLY: reproducible from a 64-bit seed (xoshiro256**, not a CSPRNG) ----
int rtfhe_packing_keygen_deterministic(const rtfhe_params* p, uint64_t seed, const int32_t* key0, const int32_t* key1, uint32_t* pk) {
    if (!valid(p) || !key0 || !key1 || !pk) return RTFHE_ERR_INVALID;
    return packing_keygen(p, Source::from_seed(seed), key0, key1, pk);
}

int rtfhe_ksk_expand_ref_deterministic(const rtfhe_params* p, uint64_t seed, const int32_t* key0, const int32_t* key1, const uint32_t* ksk, uint32_t* ksk_ref) {
    if (!valid(p) || !key0 || !key1 || !ksk || !ksk_ref) return RTFHE_ERR_INVALID;
    return ksk_expand_ref(p, Source::from_seed(seed), key0, key1, ksk, ksk_ref);
}

int rtfhe_keygen_deterministic(const rtfhe_params* p, uint64_t seed, int32_t* key0, int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    Xoshiro root(seed);
    for (int i = 0; i < p->n; i++) key0[i] = (int32_t)(root.next() >> 63);
    for (int i = 0; i < p->N; i++) key1[i] = (int32_t)(root.next() >> 63);
    return keygen_material(p, Source::from_seed(root.next()), key0, key1, bk, ksk);
}

int rtfhe_keygen_with_keys_deterministic(const rtfhe_params* p, uint64_t seed, const int32_t* key0, const int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    return keygen_material(p, Source::from_seed(seed), key0, key1, bk, ksk);
}

int rtfhe_tlwe_encrypt_bits_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t seed, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !bits || !out) return RTFHE_ERR_INVALID;
    Xoshiro r(seed);
    return encrypt_bits(p, r, key0, bits, out, count);
}

int rtfhe_tlwe_encrypt_torus_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t seed, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !mu || !out) return RTFHE_ERR_INVALID;
    Xoshiro r(seed);
    return encrypt_torus(p, r, key0, mu, out, count);
}

int rtfhe_trlwe_encrypt_torus_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t seed, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    Xoshiro r(seed);
    return encrypt_trlwe(p, r, key1, mu, out, count);
}

int rtfhe_trgsw_encrypt_bits_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t seed, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !bits || !out) return RTFHE_ERR_INVALID;
    Xoshiro r(seed);
    return encrypt_trgsw_bits(p, r, key1, bits, out, count);
}

int rtfhe_trgsw_encrypt_polys_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t seed, const int32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    Xoshiro r(seed);
    return encrypt_trgsw_polys(p, r, key1, mu, out, count);
}

// phase = b - a * s (exact negacyclic product with the binary key), per TRLWE of ct[count][2][N]
int rtfhe_trlwe_phase(const rtfhe_params* p, const int32_t* key1, const uint32_t* ct, uint32_t* phase, size_t count) {
    if (!valid(p) || !key1 || !ct || !phase) return RTFHE_ERR_INVALID;
    const int N = p->N;
    for (int i = 0; i < N; i++) if (key1[i] != 0 && key1[i] != 1) return RTFHE_ERR_INVALID;
    for (size_t g = 0; g < count; g++) {
        const uint32_t* b = ct + g * 2 * (size_t)N;
        const uint32_t* a = b + N;
        uint32_t* ph = phase + g * (size_t)N;
        std::memcpy(ph, b, (size_t)N * 4);
        for (int j = 0; j < N; j++) {
            if (!key1[j]) continue;
            for (int k = 0; k < N - j; k++) ph[k + j] -= a[k];
            for (int k = N - j; k < N; k++) ph[k + j - N] += a[k];
        }
    }
    return 0;
}

int rtfhe_tlwe_phase(const rtfhe_params* p, const int32_t* key0, const uint32_t* in, uint32_t* phase, size_t count) {
    if (!valid(p) || !key0 || !in || !phase) return RTFHE_ERR_INVALID;
    for (size_t g = 0; g < count; g++) {
        const uint32_t* ct = in + g * ((size_t)p->n + 1);
        uint32_t s = 0;
        for (int i = 0; i < p->n; i++) if (key0[i]) s += ct[i];
        phase[g] = ct[p->n] - s;
    }
    return 0;
}

int rtfhe_tlwe_decrypt_bits(const rtfhe_params* p, const int32_t* key0, const uint32_t* in, uint8_t* bits, size_t count) {
    if (!valid(p) || !key0 || !in || !bits) return RTFHE_ERR_INVALID;
    std::vector<uint32_t> ph(count);
    if (int rc = rtfhe_tlwe_phase(p, key0, in, ph.data(), count)) return rc;
    // torus2binary (tlwe.rs:187-194): One iff f32(t) * 2^-32 < 0.5
    for (size_t g = 0; g < count; g++) bits[g] = ((float)ph[g] * (1.0f / 4294967296.0f) < 0.5f) ? 1 : 0;
    return 0;
}

}  // extern "C"
