// rtfhe_dispatch_ntt.hip -- the exact-integer NTT backend (rtfhe_ntt.hpp): host tables, the NTT-domain key, kernel shapes per batch.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_ntt.hpp"
#include "rtfhe_kernels_ntt_halves.hpp"
#include "rtfhe_kernels_ntt_wg.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// ---- exact-integer NTT backend: host tables (rtfhe_ntt.hpp; validated by scripts/ntt/model.py) ----
typedef unsigned __int128 u128;
uint64_t mulmod_p(uint64_t a, uint64_t b) { return (uint64_t)((u128)a * b % ntt::P_U64); }
uint64_t powmod_p(uint64_t a, uint64_t e) { uint64_t r = 1; while (e) { if (e & 1) r = mulmod_p(r, a); a = mulmod_p(a, a); e >>= 1; } return r; }
double centred_p(uint64_t x) { return x > ntt::P_U64 / 2 ? -(double)(ntt::P_U64 - x) : (double)x; }
int bitrev(int x, int bits) { int r = 0; for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i); return r; }

// z[k], k = 1..1023: the block twiddles of a 1024-point wave transform, k = (blocks of the stage) + block;
// device order: pass 1 [15], pass 2 [15][16], pass 3 [12][64]
void ntt_fill_table(double* d, const std::vector<uint64_t>& z) {
    for (int e = 0; e < 15; e++) d[ntt::TW_P1 + e] = centred_p(z[e + 1]);
    for (int mb = 3; mb >= 0; mb--) {
        const int nb = 8 >> mb;
        for (int idx = 0; idx < nb; idx++)
            for (int B = 0; B < 16; B++)
                d[ntt::TW_P2 + (nb - 1 + idx) * 16 + B] = centred_p(z[(128 >> mb) + (B << (3 - mb)) + idx]);
    }
    for (int v = 0; v < 64; v++) {
        for (int e = 0; e < 4; e++) d[ntt::TW_P3 + e * 64 + v] = centred_p(z[256 + 4 * v + e]);
        for (int e = 0; e < 8; e++) d[ntt::TW_P3 + (4 + e) * 64 + v] = centred_p(z[512 + 8 * v + e]);
    }
}

// digit table: entry e = (e as a signed 6-bit value) * c mod P, centred
void ntt_fill_digits(double* d, uint64_t zeta1) {
    for (int e = 0; e < ntt::DIGITS; e++) {
        const int sdig = e < ntt::DIGITS / 2 ? e : e - ntt::DIGITS;
        const uint64_t mag = mulmod_p((uint64_t)(sdig < 0 ? -sdig : sdig), zeta1);
        d[e] = centred_p(sdig < 0 ? (ntt::P_U64 - mag) % ntt::P_U64 : mag);
    }
}

// N = 1024: zeta_k = psi^bitrev(k), psi a primitive 2048-th root of unity (22 generates F_P^*)
std::vector<double> ntt_device_table() {
    const uint64_t psi = powmod_p(22, (ntt::P_U64 - 1) / (2 * ntt::N));
    std::vector<uint64_t> zeta(ntt::N), zinv(ntt::N);
    for (int k = 1; k < ntt::N; k++) { zeta[k] = powmod_p(psi, (uint64_t)bitrev(k, 10)); zinv[k] = powmod_p(zeta[k], ntt::P_U64 - 2); }
    std::vector<double> t(ntt::TW_TOTAL, 0.0);
    ntt_fill_table(t.data(), zeta);
    ntt_fill_table(t.data() + ntt::TW_DIR_PAD, zinv);
    // the five digit tables of the first two stages: zeta_1; zeta_2, zeta_3 (the two blocks of stage 2); zeta_2 zeta_1, zeta_3 zeta_1
    const uint64_t coeff[ntt::DIG_TABLES] = {zeta[1], zeta[2], zeta[3], mulmod_p(zeta[2], zeta[1]), mulmod_p(zeta[3], zeta[1])};
    for (int k = 0; k < ntt::DIG_TABLES; k++) ntt_fill_digits(t.data() + ntt::TW_DIG + k * ntt::DIGITS, coeff[k]);
    return t;
}

// N = 2048 (rtfhe_kernels_ntt_halves.hpp; scripts/ntt/model2048.py): [half][1024] forward tables; the 1024-point transform of
// half H uses zeta_{k' + (1 + H) 2^floor(log2 k')} of the 2048-point table; the pad entry holds zeta_1 (the stage across the halves)
std::vector<double> ntt_halves_device_table() {
    constexpr int N2 = 2048;
    const uint64_t psi = powmod_p(22, (ntt::P_U64 - 1) / (2 * N2));
    std::vector<uint64_t> zeta(N2);
    for (int k = 1; k < N2; k++) zeta[k] = powmod_p(psi, (uint64_t)bitrev(k, 11));
    std::vector<double> t(NttHalvesTw::TOTAL, 0.0);
    for (int H = 0; H < 2; H++) {
        std::vector<uint64_t> sub(ntt::N);
        for (int kp = 1; kp < ntt::N; kp++) {
            int top = 0; while ((2 << top) <= kp) top++;
            sub[kp] = zeta[kp + ((1 + H) << top)];
        }
        double* d = t.data() + (size_t)H * NttHalvesTw::TABLE;
        ntt_fill_table(d, sub);
        d[NttHalvesTw::CROSS] = centred_p(zeta[1]);
    }
    ntt_fill_digits(t.data() + NttHalvesTw::DIG, zeta[1]);
    return t;
}

// ---- the kernel shapes of this backend (Shape / Family: rtfhe_host.hpp) ----
template <int W>
struct NttWaveShape : GatesPerWorkgroup<W, 64> {        // one wave per gate, W gates per workgroup (rtfhe_kernels_ntt.hpp)
    static GateKernel<NttBootstrapArgs> kernels() { return {k_bootstrap_ntt<3, 6, 8, 2, KSQ, W>}; }
    static constexpr size_t lds(int npad) { return ntt_lds_bytes(W, npad); }
    static NttBootstrapArgs args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_ntt_tw, ctx->d_ntt_bk}; }
};
template <int GATES>
struct NttPairShape : GatesPerWorkgroup<GATES, 128> {   // two waves per gate
    static GateKernel<NttBootstrapArgs> kernels() { return {k_bootstrap_ntt_pair<3, 6, 8, 2, KSQ, GATES>}; }
    static constexpr size_t lds(int npad) { return NttPairLds::bytes(GATES, npad); }
    static NttBootstrapArgs args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_ntt_tw, ctx->d_ntt_bk}; }
};
template <int GATES>
struct NttWgShape : GatesPerWorkgroup<GATES, 512> {     // one gate per 8-wave workgroup, the latency shape (rtfhe_kernels_ntt_wg.hpp)
    static GateKernel<NttBootstrapArgs> kernels() { return {k_bootstrap_ntt_wg<3, 6, 8, 2, KSQ>}; }
    static constexpr size_t lds(int npad) { return NttWgLds::bytes(npad); }
    static NttBootstrapArgs args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_ntt_tw, ctx->d_ntt_bk}; }
};
template <int GATES>
struct NttHalvesShape : GatesPerWorkgroup<GATES, 128> { // N = 2048: two waves per gate, one per half of the transform (rtfhe_kernels_ntt_halves.hpp)
    static GateKernel<NttHalvesArgs> kernels() { return {k_bootstrap_ntt_halves<3, 6, 8, 2, KSQ, GATES>}; }
    static constexpr size_t lds(int npad) { return NttHalvesLds::bytes(GATES, npad); }
    static NttHalvesArgs args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_ntt_tw, ctx->d_ntt_bk}; }
};
typedef Family<NttWaveShape, 4> NttWave;
typedef Family<NttPairShape, 1, 2, 3, 4> NttPair;
typedef Family<NttWgShape, 1> NttWg;
typedef Family<NttHalvesShape, 1, 2, 3, 4> NttHalves;

// Every (kernel family, gates per workgroup) the dispatch can launch fits the CU's LDS at the longest mask the context accepts
static_assert(NttPair::fits(NPAD_MAX) && NttWave::fits(NPAD_MAX) && NttWg::fits(NPAD_MAX) && NttHalves::fits(NPAD_MAX), "every shape at every mask length");

}  // namespace

namespace rtfhe_host {

int ntt_prepare(rtfhe_ctx* ctx) {
    if (ctx->ntt_ready) return 0;
    if (!ctx->d_bk_torus) return fail(ctx, RTFHE_ERR_STATE, "the NTT backend needs the bootstrapping key in torus form (rtfhe_load_bk_torus)");
    const bool halves = ctx->logn == 11;
    if (!ctx->d_ntt_tw) {
        std::vector<double> t = halves ? ntt_halves_device_table() : ntt_device_table();
        HIPCHECK(ctx, hipMalloc((void**)&ctx->d_ntt_tw, t.size() * sizeof(double)));
        HIPCHECK(ctx, hipMemcpy(ctx->d_ntt_tw, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    const size_t words = bk_word_count(ctx->p);
    if (!ctx->d_ntt_bk) HIPCHECK(ctx, hipMalloc((void**)&ctx->d_ntt_bk, words * sizeof(double)));
    constexpr int W = 4;
    const int32_t polys = (int32_t)(words / ctx->p.N);
    const double ninv = centred_p(powmod_p((uint64_t)ctx->p.N, ntt::P_U64 - 2));
    int grid = (polys + W - 1) / W; if (grid > 2048) grid = 2048;
    if (int rc = halves ? launch_kernel(ctx, k_ntt_bk_halves<W>, dim3(grid), dim3(64 * W), (size_t)(NttHalvesTw::TOTAL + W * ntt::XSLOTS) * sizeof(double), ctx->stream,
                                        NttHalvesBkArgs{ctx->d_ntt_tw, ctx->d_bk_torus, ctx->d_ntt_bk, polys, 2 * ctx->p.l, ninv}, false)
                        : launch_kernel(ctx, k_ntt_bk<W>, dim3(grid), dim3(64 * W), (size_t)(ntt::TW_DIR_PAD + W * ntt::XSLOTS) * sizeof(double), ctx->stream,
                                        NttBkArgs{ctx->d_ntt_tw, ctx->d_bk_torus, ctx->d_ntt_bk, polys, 2 * ctx->p.l, ninv}, false))
        return rc;
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->ntt_ready = true;
    return 0;
}

// Two waves per gate: 11.5 ms per 1024 gates vs 13.3 ms one wave per gate in 4-wave workgroups (RTFHE_FORCE_WAVES=4, N = 1024 only); 6-wave
// workgroups of the latter measured slower still (64 k vs 76 k gates/s): LDS-bound.  Both rings walk the ladder in rounds of 4 gates per CU; at
// N = 1024 a tail of at most one gate per CU takes the latency shape (RTFHE_FORCE_WAVES=2: stays on two waves per gate).
int launch_bootstrap_ntt(rtfhe_ctx* ctx, BootstrapArgs a, hipStream_t s) {
    if (ctx->logn == 10 && ctx->force_waves == 4) return NttWave::launch(ctx, 4, a, s);
    return walk_ladder(ctx, a, s, LutRef{}, 4, false, [&](const BootstrapArgs& b, const LutRef&, int gates, bool tail) {
        if (ctx->logn == 11) return NttHalves::launch(ctx, gates, b, s);
        return tail && gates == 1 && ctx->force_waves != 2 ? NttWg::launch(ctx, 1, b, s) : NttPair::launch(ctx, gates, b, s);
    });
}

// external product of `count` TRLWE samples with bk[idx[g]] on the NTT backend (stage-level entry point)
int launch_extprod_ntt(rtfhe_ctx* ctx, const int32_t* d_idx, const uint32_t* d_in, uint32_t* d_out, int32_t count, hipStream_t s) {
    if (ctx->logn == 11) {
        const size_t lds = NttHalvesLds::TW + (size_t)2 * 2048 * 4 + 2 * NttHalvesLds::XB;
        return launch_kernel(ctx, k_external_product_ntt_halves<3, 6>, dim3(count), dim3(128), lds, s, NttHalvesExtProdArgs{ctx->d_ntt_tw, ctx->d_ntt_bk, d_idx, d_in, d_out, count}, false);
    }
    constexpr int W = 4;
    return launch_kernel(ctx, k_external_product_ntt<3, 6, W>, dim3((count + W - 1) / W), dim3(64 * W), ntt_lds_bytes(W, 0), s, NttExtProdArgs{ctx->d_ntt_tw, ctx->d_ntt_bk, d_idx, d_in, d_out, count}, false);
}

int prime_ntt_kernels(rtfhe_ctx* ctx) {
    const int npad = (ctx->p.n + 1 + 63) / 64 * 64;
    if (ctx->logn == 11) return NttHalves::prime(ctx, npad);
    if (int rc = NttPair::prime(ctx, npad)) return rc;
    if (int rc = NttWave::prime(ctx, npad)) return rc;
    return NttWg::prime(ctx, npad);
}

}  // namespace rtfhe_host
