// rtfhe_sampling.hpp -- host only: the random generators and the torus samplers behind the host-side key generation and encryption: what the
// encryptor core (rtfhe_encrypt.hpp) of rtfhe_keygen.cpp and rtfhe_seeded.cpp draws every noise sample and forms every message word with.
//   torus!(f32)                utils/src/math.rs:691-696
// Randomness.  The reference draws every mask, noise sample and key bit from rand::thread_rng (a ChaCha-based CSPRNG seeded from the OS;
// utils/src/math.rs:417-479).  The production entry points do the same: a 256-bit key from getrandom(2) (falling back to /dev/urandom), expanded
// with ChaCha20 (rtfhe_chacha.hpp), one independent stream (nonce) per key row.  The *_deterministic entry points expand a caller-supplied 64-bit
// seed through xoshiro256** -- NOT a CSPRNG, reproducible by anyone who knows the seed: fixtures, tests and benchmarks only.
#pragma once

#include <sys/random.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/rtfhe.h"
#include "rtfhe_chacha.hpp"

namespace rtfhe_sampling {

struct Rng {
    virtual ~Rng() = default;
    virtual uint64_t next() = 0;
    float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }
    double unit53() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

// TEST ONLY: xoshiro256** seeded through splitmix64
struct Xoshiro final : Rng {
    uint64_t s[4];
    static uint64_t splitmix(uint64_t& x) {
        uint64_t z = (x += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    explicit Xoshiro(uint64_t seed) { for (auto& v : s) v = splitmix(seed); }
    static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
    uint64_t next() override {
        const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
        s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
        return r;
    }
};

// ChaCha20 keystream (RFC 8439 2.3): 256-bit key, 64-bit block counter, 64-bit stream id in the nonce words
struct ChaCha final : Rng {
    uint32_t key[8]; uint64_t stream, counter = 0; uint32_t block[16]; int used = 16;
    ChaCha(const uint32_t (&k)[8], uint64_t stream_id) : stream(stream_id) { std::memcpy(key, k, sizeof(key)); }
    ~ChaCha() override { volatile uint32_t* p = key; for (int i = 0; i < 8; i++) p[i] = 0; }
    void refill() {
        rtfhe::chacha_block(key, counter, stream, block);
        counter++; used = 0;
    }
    uint64_t next() override {
        if (used >= 16) refill();
        const uint64_t v = (uint64_t)block[used] | ((uint64_t)block[used + 1] << 32);
        used += 2;
        return v;
    }
};

inline bool os_random(void* buf, size_t len) {
    unsigned char* p = (unsigned char*)buf;
    size_t got = 0;
    while (got < len) {
        const ssize_t r = getrandom(p + got, len - got, 0);
        if (r <= 0) break;
        got += (size_t)r;
    }
    if (got == len) return true;
    FILE* f = std::fopen("/dev/urandom", "rb");
    if (!f) return false;
    const size_t r = std::fread(p, 1, len, f);
    std::fclose(f);
    return r == len;
}

// where the per-row generators come from: a seed (test only) or a ChaCha key from the OS
struct Source {
    bool secure = false; uint64_t seed = 0; uint32_t key[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    ~Source() { volatile uint32_t* p = key; for (int i = 0; i < 8; i++) p[i] = 0; }      // the ChaCha key does not outlive the call
    static bool from_os(Source& s) { s.secure = true; return os_random(s.key, sizeof(s.key)); }
    static Source from_seed(uint64_t seed) { Source s; s.seed = seed; return s; }
    Source() = default;
    Source(const Source&) = default;
};

inline uint32_t torus_from_f32(float v) {
    volatile float w = v - std::floor(v);
    volatile float fr = w - std::trunc(w);
    volatile float x = fr * 4294967296.0f;
    if (!(x > 0.0f)) return 0u;
    if (x >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)x;
}
inline uint32_t uniform_torus(Rng& r) { return torus_from_f32(r.unit()); }
inline uint32_t gaussian_torus(Rng& r, float alpha) {
    double u1 = r.unit53(), u2 = r.unit53();
    if (u1 < 1e-300) u1 = 1e-300;
    const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
    return torus_from_f32((float)z * alpha);
}

// The same distribution without the f32 round trip: z alpha 2^32 rounded to the nearest integer in double precision.  torus_from_f32 above
// truncates towards zero on the positive side and rounds 1 + v to f32's 2^-24 grid on the negative side, which leaves the samples of
// alpha = 2^-25 with a mean of about +10 LSB (2^-28.7).  One row does not notice; the packing key switch adds n t P rep ~ 4 * 10^6 such
// samples into every coefficient, where a common mean grows linearly, so the packing key's rows are drawn with this one.
inline uint32_t gaussian_torus_centred(Rng& r, double alpha) {
    double u1 = r.unit53(), u2 = r.unit53();
    if (u1 < 1e-300) u1 = 1e-300;
    const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2);
    return (uint32_t)(int64_t)std::llround(z * alpha * 4294967296.0);
}

// the message words of the gadget rows and of the packing / key-switching keys, formed in f32 as the reference forms them
inline uint32_t trgsw_bit_share(int32_t mu, int bgbit, int k) {      // mu / Bg^(k+1) (trgsw.rs:217-229)
    const float bg_inv = 1.0f / (float)(1 << bgbit);
    float pw = 1.0f;
    for (int e = 0; e < 1 + k; e++) pw *= bg_inv;
    return torus_from_f32((float)mu * pw);
}
inline uint32_t ks_digit_share(int32_t key_bit, int basebit, int lv, int d) {      // (d + 1) key_bit / 2^(basebit (lv + 1)) (tlwe.rs:252-274)
    float pw = 1.0f;
    for (int e = 0; e < basebit * (lv + 1); e++) pw *= 0.5f;
    return torus_from_f32((float)key_bit * pw * (float)(d + 1));
}

inline bool valid(const rtfhe_params* p) {
    return p && p->n > 0 && p->N >= 16 && (p->N & (p->N - 1)) == 0 && p->l > 0 && p->bgbit > 0 && p->l * p->bgbit <= 32 &&
           p->ks_t > 0 && p->ks_basebit > 0 && p->ks_t * p->ks_basebit <= 32;
}

}  // namespace rtfhe_sampling
