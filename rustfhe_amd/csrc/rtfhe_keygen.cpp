// rtfhe_keygen.cpp -- host-side key generation and TLWE encryption/decryption behind the C ABI: the unseeded entry points, the phase functions
// and decrypt.  Off the timed path (the reference's TFHE::new is setup too, hom_nand/src/tfhe.rs:21-25), kept on the host like the reference's.
// Every row is made by the encryptor core of rtfhe_encrypt.hpp with the mask drawn from the noise generator (DrawnMask); the seeded entry points
// of rtfhe_seeded.cpp run the same core with the mask from a public seed.  Follows besides:
//   TLWE decrypt               hom_nand/src/tlwe.rs:181-241
//   BootstrappingKey::new      hom_nand/src/tfhe.rs:119-126 (torus form; the device transforms it)
//   KeySwitchingKey::new       hom_nand/src/tlwe.rs:247-277
// Randomness, the generators and the torus samplers: rtfhe_sampling.hpp; the ChaCha20 block function: rtfhe_chacha.hpp.
// What is refused: the unseeded entry points need only valid(p) (the seeded ring-row ones also N in [16, 2048]); count = 0 is a no-op.
#include "../../include/rtfhe.h"

#include <cstring>
#include <vector>

#include "rtfhe_encrypt.hpp"
#include "rtfhe_mb_plan.h"
#include "rtfhe_trlwe_auto_plan.h"

namespace {

using namespace rtfhe_encrypt;

const DrawnMask DRAWN{};

// key material for given secret keys (TFHE::new, hom_nand/src/tfhe.rs:21-25); one generator per TRGSW (secure: ChaCha domain 1) / per KSK
// coefficient
int keygen_material(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!binary(key0, p->n) || !binary(key1, p->N)) return RTFHE_ERR_INVALID;
    const size_t trgsw = (size_t)2 * 2 * p->l * p->N;
    if (bk)
        striped(src, 1, root_word(src, 1), 0x9e3779b97f4a7c15ull, p->n,
                [&](Rng& r, int i) { trgsw_rows(r, DRAWN, 0, p, key1, BitShare(p, key0[i]), bk + (size_t)i * trgsw, nullptr); });
    if (ksk) ksk_keygen(p, src, DRAWN, key0, key1, ksk);
    return 0;
}

// The multi-bit bootstrapping key (include/rtfhe.h: rtfhe_mbk_keygen): key0's bits in groups of g, group t = bits [t g, min(n, t g + g)); a group
// of g' bits holds a TRGSW sample under key1 for every non-empty subset j = 1 .. 2^g' - 1 of its bits (bit q of j = bit t g + q of the key), a
// sample of the constant  prod_{q in j} s_q  prod_{q not in j} (1 - s_q)  -- exactly one of them 1, unless every bit of the group is 0.  Each is
// a bootstrapping-key entry in everything else: the same gadget, the same noise, the same rows from the encryptor core.  Groups in order, j
// ascending; one generator per sample (secure: ChaCha domain 5).
int mbk_material(const rtfhe_params* p, const Source& src, int32_t g, const int32_t* key0, const int32_t* key1, uint32_t* out) {
    const int64_t total = rtfhe_mb_trgsw_count(p->n, g);
    if (total < 0 || total > 0x7fffffff || !binary(key0, p->n) || !binary(key1, p->N)) return RTFHE_ERR_INVALID;
    const size_t trgsw = (size_t)2 * 2 * p->l * p->N;
    const int J = (1 << g) - 1, full = p->n / g;
    striped(src, 5, root_word(src, 4), 0xda942042e4dd58b5ull, (int)total, [&](Rng& r, int e) {
        const int t = e < full * J ? e / J : full, j = e - t * J + 1, bits = t < full ? g : p->n % g;
        int32_t mu = 1;
        for (int q = 0; q < bits; q++) mu &= ((j >> q) & 1) ? key0[t * g + q] : 1 - key0[t * g + q];
        trgsw_rows(r, DRAWN, 0, p, key1, BitShare(p, mu), out + (size_t)e * trgsw, nullptr);
    });
    return 0;
}

// The TRLWE switching key (include/rtfhe.h: rtfhe_trlwe_ksk_keygen): entry e holds, for every gadget position j, a TRLWE row under key_to of
// -sigma_{t[e]}(key_from) * 2^(32 - (j+1) bgbit) -- a zero encryption from the encryptor core, as a bootstrapping-key row, plus that message on b.
// Entries in order, j ascending; one generator per entry (secure: ChaCha domain 6).  The exponent rules: rtfhe_trlwe_auto_exponents_bad (rtfhe_trlwe_auto_plan.h).
int trlwe_ksk_material(const rtfhe_params* p, const Source& src, const int32_t* key_from, const int32_t* key_to, const int32_t* t, int32_t n_t, uint32_t* out) {
    if (rtfhe_trlwe_auto_exponents_bad(p->N, t, n_t) || !binary(key_from, p->N) || !binary(key_to, p->N)) return RTFHE_ERR_INVALID;
    const int N = p->N;
    striped(src, 6, root_word(src, 5), 0xa0761d6478bd642full, n_t, [&](Rng& r, int e) {
        std::vector<uint32_t> k((size_t)N), s((size_t)N);
        for (int c = 0; c < N; c++) k[c] = (uint32_t)key_from[c];
        rtfhe_trlwe_auto_permute(N, t[e], k.data(), s.data());      // sigma_t(key_from): +-1 and 0 as wrapping words
        uint32_t* rows = out + (size_t)e * p->l * 2 * N;
        for (int j = 0; j < p->l; j++) {
            uint32_t* b = trlwe_row(r, DRAWN, (uint64_t)j, N, key_to, false, rows, nullptr);
            for (int c = 0; c < N; c++) b[c] -= s[c] << (32 - (j + 1) * p->bgbit);
        }
    });
    return 0;
}

void draw_keys(const rtfhe_params* p, Rng& r, int32_t* key0, int32_t* key1) {
    for (int i = 0; i < p->n; i++) key0[i] = (int32_t)(r.next() >> 63);
    for (int i = 0; i < p->N; i++) key1[i] = (int32_t)(r.next() >> 63);
}

// rtfhe_packing_keygen* refuse non-binary keys and ks parameters other than (8, 2), the one instantiation the packing key switch has
int packing_key(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, uint32_t* pk) {
    if (p->ks_t != 8 || p->ks_basebit != 2 || !binary(key0, p->n) || !binary(key1, p->N)) return RTFHE_ERR_INVALID;
    return packing_keygen(p, src, DRAWN, key0, key1, pk);
}

// The reference's container shape from the compact one: [N][t][base][n+1] with entries 0 .. base-2 of every level copied and entry
// base-1 = TLWE(base * s_i / 2^(basebit (l+1))) freshly encrypted, as KeySwitchingKey::new fills it (hom_nand/src/tlwe.rs:252-274).
// One generator per coefficient (secure: ChaCha domain 3), in turn.
int ksk_expand_ref(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, const uint32_t* ksk, uint32_t* ksk_ref) {
    const int n = p->n, t = p->ks_t, bb = p->ks_basebit, base = 1 << bb;
    if (!binary(key0, n) || !binary(key1, p->N)) return RTFHE_ERR_INVALID;
    const size_t w = (size_t)n + 1;
    for (int i = 0; i < p->N; i++)
        coefficient_rng(src, 3, src.seed, 0x94d049bb133111ebull, i, [&](Rng& r) {
            for (int lv = 0; lv < t; lv++) {
                const size_t il = (size_t)i * t + lv;
                std::memcpy(ksk_ref + il * base * w, ksk + il * (base - 1) * w, (size_t)(base - 1) * w * sizeof(uint32_t));
                tlwe_row(r, DRAWN, il * base + (base - 1), n, key0, ks_digit_share(key1[i], bb, lv, base - 1), ksk_ref, nullptr);
            }
        });
    return 0;
}

// rtfhe_tlwe_encrypt_bits/torus[_deterministic] do not check that key0 is binary (any non-zero word counts as 1, as in rtfhe_tlwe_phase); the
// seeded lvl0 encryptors, keygen_with_keys, the packing key and every lvl1 encryptor refuse a non-binary key
int encrypt_bits(const rtfhe_params* p, Rng& r, const int32_t* key0, const uint8_t* bits, uint32_t* out, size_t count) {
    return encrypt_tlwe(r, DRAWN, p, key0, [&](size_t g) { return bit_word(bits[g]); }, out, count);
}

// the same with the plaintext torus words given directly (multi-bit messages for the programmable bootstrap)
int encrypt_torus(const rtfhe_params* p, Rng& r, const int32_t* key0, const uint32_t* mu, uint32_t* out, size_t count) {
    return encrypt_tlwe(r, DRAWN, p, key0, [&](size_t g) { return mu[g]; }, out, count);
}

// the lvl1 encryptors (rtfhe_encrypt.hpp) of a binary key1: encrypted tables [count][2][N] (rtfhe_lut_create_encrypted), the selectors of a CMUX
// tree [count][2][2l][N] (rtfhe_trgsw_create: what keygen_material does per key bit), encrypted weights (rtfhe_trlwe_mul_trgsw_batch)
template <class In, class Encrypt>
int encrypt_lvl1(const rtfhe_params* p, Rng& r, const int32_t* key1, const In* in, uint32_t* out, size_t count, Encrypt encrypt) {
    if (!binary(key1, p->N)) return RTFHE_ERR_INVALID;
    return encrypt(r, DRAWN, p, key1, in, out, count);
}
int encrypt_trlwe_torus(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint32_t* mu, uint32_t* out, size_t count) {
    return encrypt_lvl1(p, r, key1, mu, out, count, encrypt_trlwe<DrawnMask>);
}
int encrypt_selectors(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint8_t* bits, uint32_t* out, size_t count) {
    return encrypt_lvl1(p, r, key1, bits, out, count, encrypt_trgsw_bits<DrawnMask>);
}
int encrypt_weights(const rtfhe_params* p, Rng& r, const int32_t* key1, const int32_t* mu, uint32_t* out, size_t count) {
    return encrypt_lvl1(p, r, key1, mu, out, count, encrypt_trgsw_polys<DrawnMask>);
}

}  // namespace

extern "C" {

// ---- production: OS CSPRNG ----
int rtfhe_keygen(const rtfhe_params* p, int32_t* key0, int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    return production_source(nullptr, [&](const Source& src) {
        { ChaCha r(src.key, 0); draw_keys(p, r, key0, key1); }
        return keygen_material(p, src, key0, key1, bk, ksk);
    });
}

int rtfhe_keygen_with_keys(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    return production_source(nullptr, [&](const Source& src) { return keygen_material(p, src, key0, key1, bk, ksk); });
}

int rtfhe_tlwe_encrypt_bits(const rtfhe_params* p, const int32_t* key0, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !bits || !out) return RTFHE_ERR_INVALID;
    return production(nullptr, [&](Rng& r) { return encrypt_bits(p, r, key0, bits, out, count); });
}

int rtfhe_tlwe_encrypt_torus(const rtfhe_params* p, const int32_t* key0, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !mu || !out) return RTFHE_ERR_INVALID;
    return production(nullptr, [&](Rng& r) { return encrypt_torus(p, r, key0, mu, out, count); });
}

int rtfhe_trlwe_encrypt_torus(const rtfhe_params* p, const int32_t* key1, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    return production(nullptr, [&](Rng& r) { return encrypt_trlwe_torus(p, r, key1, mu, out, count); });
}

int rtfhe_trgsw_encrypt_bits(const rtfhe_params* p, const int32_t* key1, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !bits || !out) return RTFHE_ERR_INVALID;
    return production(nullptr, [&](Rng& r) { return encrypt_selectors(p, r, key1, bits, out, count); });
}

int rtfhe_trgsw_encrypt_polys(const rtfhe_params* p, const int32_t* key1, const int32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    return production(nullptr, [&](Rng& r) { return encrypt_weights(p, r, key1, mu, out, count); });
}

int rtfhe_ksk_expand_ref(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, const uint32_t* ksk, uint32_t* ksk_ref) {
    if (!valid(p) || !key0 || !key1 || !ksk || !ksk_ref) return RTFHE_ERR_INVALID;
    return production_source(nullptr, [&](const Source& src) { return ksk_expand_ref(p, src, key0, key1, ksk, ksk_ref); });
}

int rtfhe_packing_keygen(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* pk) {
    if (!valid(p) || !key0 || !key1 || !pk) return RTFHE_ERR_INVALID;
    return production_source(nullptr, [&](const Source& src) { return packing_key(p, src, key0, key1, pk); });
}

int rtfhe_mbk_keygen(const rtfhe_params* p, int32_t g, const int32_t* key0, const int32_t* key1, uint32_t* out) {
    if (!valid(p) || !key0 || !key1 || !out) return RTFHE_ERR_INVALID;
    return production_source(nullptr, [&](const Source& src) { return mbk_material(p, src, g, key0, key1, out); });
}

int rtfhe_trlwe_ksk_keygen(const rtfhe_params* p, const int32_t* key_from, const int32_t* key_to, const int32_t* t, int32_t n_t, uint32_t* out) {
    if (!valid(p) || !key_from || !key_to || !t || !out) return RTFHE_ERR_INVALID;
    return production_source(nullptr, [&](const Source& src) { return trlwe_ksk_material(p, src, key_from, key_to, t, n_t, out); });
}

// sigma_t on count polynomials: coefficient j goes to j t mod 2N, negated past N (the permutation the switching key's messages are made with,
// rtfhe_trlwe_auto_plan.h).  `x` may be exactly `out`.
int rtfhe_trlwe_automorphism(int32_t N, int32_t t, const uint32_t* x, uint32_t* out, size_t count) {
    if (!x || !out || !rtfhe_trlwe_auto_ring_ok(N) || !rtfhe_trlwe_auto_exponent_ok(N, t)) return RTFHE_ERR_INVALID;
    std::vector<uint32_t> tmp((size_t)N);
    for (size_t g = 0; g < count; g++) {
        rtfhe_trlwe_auto_permute(N, t, x + g * (size_t)N, tmp.data());
        std::memcpy(out + g * (size_t)N, tmp.data(), (size_t)N * sizeof(uint32_t));
    }
    return 0;
}

// ---- TEST ONLY: reproducible from a 64-bit seed (xoshiro256**, not a CSPRNG) ----
int rtfhe_trlwe_ksk_keygen_deterministic(const rtfhe_params* p, const int32_t* key_from, const int32_t* key_to, uint64_t seed, const int32_t* t, int32_t n_t,
                                         uint32_t* out) {
    if (!valid(p) || !key_from || !key_to || !t || !out) return RTFHE_ERR_INVALID;
    return trlwe_ksk_material(p, Source::from_seed(seed), key_from, key_to, t, n_t, out);
}

int rtfhe_mbk_keygen_deterministic(const rtfhe_params* p, uint64_t seed, int32_t g, const int32_t* key0, const int32_t* key1, uint32_t* out) {
    if (!valid(p) || !key0 || !key1 || !out) return RTFHE_ERR_INVALID;
    return mbk_material(p, Source::from_seed(seed), g, key0, key1, out);
}

int rtfhe_packing_keygen_deterministic(const rtfhe_params* p, uint64_t seed, const int32_t* key0, const int32_t* key1, uint32_t* pk) {
    if (!valid(p) || !key0 || !key1 || !pk) return RTFHE_ERR_INVALID;
    return packing_key(p, Source::from_seed(seed), key0, key1, pk);
}

int rtfhe_ksk_expand_ref_deterministic(const rtfhe_params* p, uint64_t seed, const int32_t* key0, const int32_t* key1, const uint32_t* ksk, uint32_t* ksk_ref) {
    if (!valid(p) || !key0 || !key1 || !ksk || !ksk_ref) return RTFHE_ERR_INVALID;
    return ksk_expand_ref(p, Source::from_seed(seed), key0, key1, ksk, ksk_ref);
}

int rtfhe_keygen_deterministic(const rtfhe_params* p, uint64_t seed, int32_t* key0, int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    return deterministic(seed, [&](Rng& root) {
        draw_keys(p, root, key0, key1);      // (first: the material's seed is the generator's next word)
        return keygen_material(p, Source::from_seed(root.next()), key0, key1, bk, ksk);
    });
}

int rtfhe_keygen_with_keys_deterministic(const rtfhe_params* p, uint64_t seed, const int32_t* key0, const int32_t* key1, uint32_t* bk, uint32_t* ksk) {
    if (!valid(p) || !key0 || !key1) return RTFHE_ERR_INVALID;
    return keygen_material(p, Source::from_seed(seed), key0, key1, bk, ksk);
}

int rtfhe_tlwe_encrypt_bits_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t seed, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !bits || !out) return RTFHE_ERR_INVALID;
    return deterministic(seed, [&](Rng& r) { return encrypt_bits(p, r, key0, bits, out, count); });
}

int rtfhe_tlwe_encrypt_torus_deterministic(const rtfhe_params* p, const int32_t* key0, uint64_t seed, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key0 || !mu || !out) return RTFHE_ERR_INVALID;
    return deterministic(seed, [&](Rng& r) { return encrypt_torus(p, r, key0, mu, out, count); });
}

int rtfhe_trlwe_encrypt_torus_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t seed, const uint32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    return deterministic(seed, [&](Rng& r) { return encrypt_trlwe_torus(p, r, key1, mu, out, count); });
}

int rtfhe_trgsw_encrypt_bits_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t seed, const uint8_t* bits, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !bits || !out) return RTFHE_ERR_INVALID;
    return deterministic(seed, [&](Rng& r) { return encrypt_selectors(p, r, key1, bits, out, count); });
}

int rtfhe_trgsw_encrypt_polys_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t seed, const int32_t* mu, uint32_t* out, size_t count) {
    if (!valid(p) || !key1 || !mu || !out) return RTFHE_ERR_INVALID;
    return deterministic(seed, [&](Rng& r) { return encrypt_weights(p, r, key1, mu, out, count); });
}

// phase = b - a * s (exact negacyclic product with the binary key), per TRLWE of ct[count][2][N]
int rtfhe_trlwe_phase(const rtfhe_params* p, const int32_t* key1, const uint32_t* ct, uint32_t* phase, size_t count) {
    if (!valid(p) || !key1 || !ct || !phase) return RTFHE_ERR_INVALID;
    const int N = p->N;
    if (!binary(key1, N)) return RTFHE_ERR_INVALID;
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

// (key0 is not checked to be binary: any non-zero word counts as 1, as in the unseeded lvl0 encryptors)
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
