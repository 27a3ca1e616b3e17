// rtfhe_seeded.cpp -- host only: seeded ciphertexts (include/rtfhe.h, "seeded ciphertexts").  The mask rule on the CPU (rtfhe_mask_expand,
// rtfhe_seeded_expand: the oracle of k_seeded_expand and the path of a server without this library's GPU side), the seeded encryptors, and the
// argument checks of every seeded call, device calls included (rtfhe_seeded_plan.h).  No HIP call in this unit.
// The encryptors draw the noise and form the message words with rtfhe_keygen.cpp's own samplers (rtfhe_sampling.hpp); only the mask differs: it
// is the ChaCha20 keystream of the public seed, all 32 bits of every word, and never the generator the noise comes from.
#include "rtfhe_seeded_plan.h"

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

std::string num(long long v) { return std::to_string(v); }

bool ring_ok(int32_t N) { return N >= 16 && N <= 2048 && (N & (N - 1)) == 0; }
// do rows first_row .. first_row + rows - 1 exist (first_row + rows <= 2^64)?
bool rows_ok(uint64_t first_row, size_t rows) { return first_row == 0 || (uint64_t)rows <= (uint64_t)0 - first_row; }

// the mask rule: row R is the keystream of stream R, blocks 0 .. N/16 - 1
void mask_row(int N, const uint32_t* seed, uint64_t R, uint32_t* a) {
    for (int c = 0; c < N / 16; c++) rtfhe::chacha_block(seed, (uint64_t)c, R, a + 16 * c);
}

bool binary(const int32_t* key, int n) {
    for (int i = 0; i < n; i++) if (key[i] != 0 && key[i] != 1) return false;
    return true;
}

// b = e + a * s (exact negacyclic product with the binary key), the noise drawn as trlwe_zero of rtfhe_keygen.cpp draws it
void masked_zero(Rng& r, int N, const int32_t* key, float alpha, bool centred, const uint32_t* a, uint32_t* b) {
    for (int k = 0; k < N; k++) b[k] = centred ? gaussian_torus_centred(r, (double)alpha) : gaussian_torus(r, alpha);
    for (int j = 0; j < N; j++) {
        if (!key[j]) continue;
        for (int k = 0; k < N - j; k++) b[k + j] += a[k];
        for (int k = N - j; k < N; k++) b[k + j - N] -= a[k];
    }
}

const float ALPHA_BK = 1.0f / 33554432.0f;   // 2^-25, trlwe.rs:77

// The b halves of one TRGSW sample whose masks are rows row0 .. row0 + 2l - 1 of the seed; share(k, c) = the message word of gadget position k at
// coefficient c.  Rows k < l carry it on b, as the unseeded encryptor places it.  Rows l + k carry it on the a polynomial, which here must stay the
// seed's keystream: the zero encryption is made under a - share, a uniform polynomial as well, so that the expanded row (b, a) is the unseeded
// encryptor's (b, (a - share) + share) word for word in form and in distribution (its phase: e - share * s).
template <typename Share>
void trgsw_b_rows(Rng& r, const rtfhe_params* p, const int32_t* key1, const uint32_t* seed, uint64_t row0, Share share, uint32_t* b, uint32_t* a) {
    const int N = p->N, l = p->l;
    for (int j = 0; j < 2 * l; j++) {
        mask_row(N, seed, row0 + (uint64_t)j, a);
        if (j >= l) for (int c = 0; c < N; c++) a[c] -= share(j - l, c);
        masked_zero(r, N, key1, ALPHA_BK, false, a, b + (size_t)j * N);
        if (j < l) for (int c = 0; c < N; c++) b[(size_t)j * N + c] += share(j, c);
    }
}

int encrypt_trlwe(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint32_t* seed, uint64_t first_row, const uint32_t* mu, uint32_t* b, size_t count) {
    const int N = p->N;
    std::vector<uint32_t> a((size_t)N);
    for (size_t g = 0; g < count; g++) {
        mask_row(N, seed, first_row + g, a.data());
        masked_zero(r, N, key1, ALPHA_BK, false, a.data(), b + g * (size_t)N);
        for (int k = 0; k < N; k++) b[g * (size_t)N + k] += mu[g * (size_t)N + k];
    }
    return 0;
}

int encrypt_trgsw_bits(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint32_t* seed, uint64_t first_row, const uint8_t* bits, uint32_t* b, size_t count) {
    const size_t rows = (size_t)2 * p->l;
    std::vector<uint32_t> a((size_t)p->N);
    for (size_t g = 0; g < count; g++) {
        uint32_t t2[32];
        for (int k = 0; k < p->l; k++) t2[k] = trgsw_bit_share(bits[g] ? 1 : 0, p->bgbit, k);
        trgsw_b_rows(r, p, key1, seed, first_row + g * rows, [&](int k, int c) { return c == 0 ? t2[k] : 0u; }, b + g * rows * (size_t)p->N, a.data());
    }
    return 0;
}

int encrypt_trgsw_polys(const rtfhe_params* p, Rng& r, const int32_t* key1, const uint32_t* seed, uint64_t first_row, const int32_t* mu, uint32_t* b, size_t count) {
    const size_t rows = (size_t)2 * p->l;
    std::vector<uint32_t> a((size_t)p->N);
    for (size_t g = 0; g < count; g++) {
        const int32_t* m = mu + g * (size_t)p->N;
        // the integer mu_c * 2^(32 - (k+1) bgbit), wrapping (>= 0 shifts: valid(p) holds l * bgbit <= 32)
        trgsw_b_rows(r, p, key1, seed, first_row + g * rows, [&](int k, int c) { return (uint32_t)m[c] << (32 - (k + 1) * p->bgbit); },
                     b + g * rows * (size_t)p->N, a.data());
    }
    return 0;
}

// rtfhe_keygen.cpp's packing_keygen with the masks from the seed: row (i, lv, d) is mask row first_row + (i t + lv)(base - 1) + d; one noise
// generator per coefficient i, striped over the threads, from the same streams (secure: ChaCha domain 4) and seeds (deterministic)
int packing_keygen(const rtfhe_params* p, const Source& src, const int32_t* key0, const int32_t* key1, const uint32_t* seed, uint64_t first_row, uint32_t* b) {
    const int n = p->n, N = p->N, t = p->ks_t, bb = p->ks_basebit, base1 = (1 << bb) - 1;
    const unsigned hw = std::thread::hardware_concurrency();
    const int nthreads = (int)(hw ? (hw > 16 ? 16 : hw) : 1);
    uint64_t s_pk = 0;
    if (!src.secure) { Xoshiro root(src.seed); root.next(); root.next(); s_pk = root.next(); }
    auto body = [&](Rng& r, int i, uint32_t* a) {
        for (int lv = 0; lv < t; lv++)
            for (int d = 0; d < base1; d++) {
                const size_t row = ((size_t)i * t + lv) * base1 + d;
                mask_row(N, seed, first_row + row, a);
                masked_zero(r, N, key1, ALPHA_BK, true, a, b + row * (size_t)N);
                b[row * (size_t)N] += ks_digit_share(key0[i], bb, lv, d);
            }
    };
    auto work = [&](int tid) {
        std::vector<uint32_t> a((size_t)N);
        for (int i = tid; i < n; i += nthreads) {
            if (src.secure) { ChaCha r(src.key, ((uint64_t)4 << 32) | (uint32_t)i); body(r, i, a.data()); }
            else { Xoshiro r(s_pk + 0xd6e8feb86659fd93ull * (uint64_t)(i + 1)); body(r, i, a.data()); }
        }
    };
    std::vector<std::thread> th;
    for (int k = 0; k < nthreads; k++) th.emplace_back(work, k);
    for (auto& x : th) x.join();
    return 0;
}

// what every seeded encryptor asks first: a valid parameter set whose ring the mask rule covers, a binary lvl1 key, rows that exist
bool encrypt_ready(const rtfhe_params* p, const int32_t* key1, const void* in, const uint32_t* seed, const void* b, uint64_t first_row, size_t count, size_t rows_each) {
    if (!valid(p) || !ring_ok(p->N) || !key1 || !in || !seed || !b) return false;
    if (rows_each && count > (size_t)-1 / rows_each) return false;
    return rows_ok(first_row, count * rows_each) && binary(key1, p->N);
}

// the production forms' two draws from the OS: the public mask seed, and -- separately -- the key of the noise generator
bool fresh(uint32_t* seed, Source& noise) { return os_random(seed, 8 * sizeof(uint32_t)) && Source::from_os(noise); }

}  // namespace

extern "C" {

int rtfhe_seeded_plan(int32_t what, int32_t N, const void* seed, uint64_t first_row, const void* b, int32_t group, const void* out, size_t rows, char* err,
                      size_t err_len) {
    if (err && err_len) err[0] = 0;
    const bool upload = what == RTFHE_SEEDED_UPLOAD;
    if (!seed || !b || (!upload && !out)) return refuse(err, err_len, "null argument");
    if (!ring_ok(N)) return refuse(err, err_len, "N = " + num(N) + " is not a power of two in [16, 2048]");
    if (group < 1) return refuse(err, err_len, "group = " + num(group) + " is below 1");
    if (rows % (size_t)group) return refuse(err, err_len, "rows = " + std::to_string(rows) + " is not a multiple of group = " + num(group));
    if (!rows_ok(first_row, rows))
        return refuse(err, err_len, "rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " + std::to_string(rows) + ") pass 2^64");
    if (what != RTFHE_SEEDED_HOST && rows > (size_t)0x7fffffff / (size_t)(N / 16)) return refuse(err, err_len, "rows * N / 16 too large (it must be below 2^31)");
    if (upload) return 0;
    const uintptr_t i0 = (uintptr_t)b, o0 = (uintptr_t)out;
    if (what == RTFHE_SEEDED_DEVICE && ((i0 | o0) & 15)) return refuse(err, err_len, "d_b and d_out must be 16-byte aligned");
    const size_t in_bytes = rows * (size_t)N * 4, out_bytes = 2 * in_bytes;
    if (i0 < o0 + out_bytes && o0 < i0 + in_bytes) return refuse(err, err_len, "the output overlaps the b rows");
    return 0;
}

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

// ---- production: the mask seed and the noise key are two draws from the OS CSPRNG; rows are numbered from 0 ----
int rtfhe_trlwe_encrypt_torus_seeded(const rtfhe_params* p, const int32_t* key1, const uint32_t* mu, uint32_t* seed, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key1, mu, seed, b, 0, count, 1)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);
    return encrypt_trlwe(p, r, key1, seed, 0, mu, b, count);
}

int rtfhe_trgsw_encrypt_bits_seeded(const rtfhe_params* p, const int32_t* key1, const uint8_t* bits, uint32_t* seed, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key1, bits, seed, b, 0, count, p ? (size_t)2 * p->l : 0)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);
    return encrypt_trgsw_bits(p, r, key1, seed, 0, bits, b, count);
}

int rtfhe_trgsw_encrypt_polys_seeded(const rtfhe_params* p, const int32_t* key1, const int32_t* mu, uint32_t* seed, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key1, mu, seed, b, 0, count, p ? (size_t)2 * p->l : 0)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    ChaCha r(src.key, 0);
    return encrypt_trgsw_polys(p, r, key1, seed, 0, mu, b, count);
}

int rtfhe_packing_keygen_seeded(const rtfhe_params* p, const int32_t* key0, const int32_t* key1, uint32_t* seed, uint32_t* b) {
    if (!encrypt_ready(p, key1, key0, seed, b, 0, 0, 0) || p->ks_t != 8 || p->ks_basebit != 2 || !binary(key0, p->n)) return RTFHE_ERR_INVALID;
    Source src;
    if (!fresh(seed, src)) return RTFHE_ERR_STATE;
    return packing_keygen(p, src, key0, key1, seed, 0, b);
}

// ---- TEST ONLY: the noise from a 64-bit seed (xoshiro256**, not a CSPRNG); the mask seed and its first row are the caller's ----
int rtfhe_trlwe_encrypt_torus_seeded_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                   const uint32_t* mu, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key1, mu, seed, b, first_row, count, 1)) return RTFHE_ERR_INVALID;
    Xoshiro r(noise_seed);
    return encrypt_trlwe(p, r, key1, seed, first_row, mu, b, count);
}

int rtfhe_trgsw_encrypt_bits_seeded_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                  const uint8_t* bits, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key1, bits, seed, b, first_row, count, p ? (size_t)2 * p->l : 0)) return RTFHE_ERR_INVALID;
    Xoshiro r(noise_seed);
    return encrypt_trgsw_bits(p, r, key1, seed, first_row, bits, b, count);
}

int rtfhe_trgsw_encrypt_polys_seeded_deterministic(const rtfhe_params* p, const int32_t* key1, uint64_t noise_seed, const uint32_t* seed, uint64_t first_row,
                                                   const int32_t* mu, uint32_t* b, size_t count) {
    if (!encrypt_ready(p, key1, mu, seed, b, first_row, count, p ? (size_t)2 * p->l : 0)) return RTFHE_ERR_INVALID;
    Xoshiro r(noise_seed);
    return encrypt_trgsw_polys(p, r, key1, seed, first_row, mu, b, count);
}

int rtfhe_packing_keygen_seeded_deterministic(const rtfhe_params* p, uint64_t noise_seed, const int32_t* key0, const int32_t* key1, const uint32_t* seed,
                                              uint64_t first_row, uint32_t* b) {
    if (!encrypt_ready(p, key1, key0, seed, b, 0, 0, 0) || p->ks_t != 8 || p->ks_basebit != 2 || !binary(key0, p->n)) return RTFHE_ERR_INVALID;
    if (!rows_ok(first_row, (size_t)p->n * 8 * 3)) return RTFHE_ERR_INVALID;
    return packing_keygen(p, Source::from_seed(noise_seed), key0, key1, seed, first_row, b);
}

}  // extern "C"
