// rtfhe_dispatch_fft.hip -- the FP64 mirror backend's bootstrap kernels and the choice of kernel shape per batch.
#include "rtfhe_host.hpp"

#include <algorithm>

#include "rtfhe_kernels_wg.hpp"
#include "rtfhe_kernels_pair.hpp"
#include "rtfhe_kernels_pair4.hpp"
#include "rtfhe_kernels_pair_rr.hpp"
#include "rtfhe_kernels_eo.hpp"
#include "rtfhe_kernels_eo4.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// ---- the kernel shapes of this backend (Shape / Family: rtfhe_host.hpp) ----
template <int LOGN, int W>
struct WaveShape : GatesPerWorkgroup<W, 64> {          // one wave per gate, W gates per workgroup (rtfhe_kernels.hpp)
    static TwinKernels<BootstrapArgs> kernels() { return RTFHE_TWINS(, LOGN, 3, 6, 8, 2, KSQ, W); }
    static constexpr size_t lds(int npad) { return bootstrap_lds_bytes<LOGN>(W, npad, bootstrap_dual_xbuf(LOGN, W)); }
    static BootstrapArgs args(const rtfhe_ctx*, const BootstrapArgs& b) { return b; }
};
template <int W> using Wave10Shape = WaveShape<10, W>;
template <int W> using Wave11Shape = WaveShape<11, W>;
template <int GATES>
struct WgShape : GatesPerWorkgroup<GATES, 512> {       // one gate per 8-wave workgroup (rtfhe_kernels_wg.hpp)
    static TwinKernels<BootstrapArgs> kernels() { return RTFHE_TWINS(_wg, 10, 3, 6, 8, 2, KSQ); }
    static constexpr size_t lds(int npad) { return WgLds<10, 3>::bytes(npad); }
    static BootstrapArgs args(const rtfhe_ctx*, const BootstrapArgs& b) { return b; }
};
template <int GATES>
struct PairShape : GatesPerWorkgroup<GATES, 128> {     // two waves per gate (rtfhe_kernels_pair.hpp)
    static TwinKernels<BootstrapArgs> kernels() { return RTFHE_TWINS(_pair, 3, 6, 8, 2, KSQ, GATES); }
    static constexpr size_t lds(int npad) { return PairLds::bytes(GATES, npad); }
    static BootstrapArgs args(const rtfhe_ctx*, const BootstrapArgs& b) { return b; }
};
template <int GATES>
struct PairRrShape : WorkgroupPerCu {                  // GATES = 5 or 6 gates on the four wave pairs of every CU, time-sliced (rtfhe_kernels_pair_rr.hpp)
    static TwinKernels<BootstrapArgs> kernels() { return RTFHE_TWINS(_pair_rr, 3, 6, 8, 2, KSQ); }
    static constexpr size_t lds(int npad) { return PairRrLds::bytes(GATES, npad); }
    static BootstrapArgs args(const rtfhe_ctx*, const BootstrapArgs& b) { return b; }
};
template <int GATES>
struct Pair4Shape : GatesPerWorkgroup<GATES, 256> {    // four waves per gate, (polynomial, parity) (rtfhe_kernels_pair4.hpp); no fused key switch
    static TwinKernels<Pair4Args> kernels() { return RTFHE_TWINS(_pair4, 3, 6, GATES); }
    static constexpr size_t lds(int npad) { return Pair4Lds::bytes(GATES, npad); }
    static Pair4Args args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_p4bk}; }
};
template <int GATES>
struct EoShape : GatesPerWorkgroup<GATES, 128> {       // N = 2048: two waves per transform, split by the parity of the point index (rtfhe_kernels_eo.hpp)
    static TwinKernels<EoArgs> kernels() { return RTFHE_TWINS(_eo, 3, 6, 8, 2, KSQ, GATES); }
    static constexpr size_t lds(int npad) { return EoLds::bytes(GATES, npad); }
    static EoArgs args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_etw, ctx->d_ebk}; }
};
template <int GATES>
struct Eo4Shape : GatesPerWorkgroup<GATES, 256> {      // N = 2048: four waves per gate, (polynomial, parity) (rtfhe_kernels_eo4.hpp); no fused key switch
    static TwinKernels<EoArgs> kernels() { return RTFHE_TWINS(_eo4, 3, 6, GATES); }
    static constexpr size_t lds(int npad) { return Eo4Lds::bytes(GATES, npad); }
    static EoArgs args(const rtfhe_ctx* ctx, const BootstrapArgs& b) { return {b, ctx->d_etw, ctx->d_ebk}; }
};
typedef Family<Wave10Shape, 4, 8> Wave10;
typedef Family<WgShape, 1> Wg;
typedef Family<PairShape, 2, 3, 4> Pair;              // (there is no pair<1>: a tail of up to one gate per CU beyond wg_max runs two per workgroup)
typedef Family<PairRrShape, 5, 6> PairRr;
typedef Family<Pair4Shape, 2, 3> Pair4;
typedef Family<Wave11Shape, 4> Wave11;
typedef Family<EoShape, 1, 2, 3, 4> Eo;
typedef Family<Eo4Shape, 1, 2> Eo4;

// 4 x CUs < count <= rr x CUs gates on the four wave pairs of every CU, time-sliced (rtfhe_kernels_pair_rr.hpp)
bool rr_applies(const rtfhe_ctx* ctx, size_t count) {
    const size_t cus = (size_t)ctx->num_cus, round = 4 * cus, rem = count % round;
    const int rr = ctx->rr > PairRrLds::GMAX ? PairRrLds::GMAX : ctx->rr;
    return rr > 4 && !ctx->force_waves && count > round && rem != 0 && round + rem <= (size_t)rr * cus;
}
// Gates per workgroup (2 or 3) of an N = 1024 tail of `rem` gates that wants four waves per gate (k_bootstrap_pair4), else 0.  k_bootstrap_pair
// would leave SIMDs a lone wave on tails of more than wg_max gates and up to two / three gates per CU (7 % on 257-512-gate and 1-4 % on
// 513-768-gate batches; at four gates per CU pair4 loses 12 %, profiles/r04/pair4_ab.log).  The dispatch and layout_needed both ask here.
int pair4_tail_gates(const rtfhe_ctx* ctx, size_t rem) {
    const size_t cus = (size_t)ctx->num_cus;
    if (rem <= (size_t)ctx->wg_max) return 0;
    const int gates = rem <= 2 * cus ? 2 : rem <= 3 * cus ? 3 : 0;
    return gates && ctx->pair4 >= gates ? gates : 0;
}
// gates per workgroup (= per CU) of the N = 2048 whole rounds: four, or three at the mask lengths where four gates' carve passes the CU's LDS
// (npad = 768, n >= 704: 163,904 bytes)
constexpr int eo_round_gates(int npad) { return EoLds::bytes(4, npad) <= LDS_LIMIT ? 4 : 3; }

// Kernel shape by batch size (N = 1024), measured in profiles/r01_pair/shape_sweep.log:
//   whole rounds of 4 gates per CU : two waves per gate, 8-wave workgroups (k_bootstrap_pair) -- best throughput at every size
//   a remainder <= 1 gate per CU   : one gate per 8-wave workgroup (k_bootstrap_wg): ~2.4x lower latency
//   a remainder <= 2 / 3 gates per CU : the two-waves-per-gate kernel with 2 / 3 gates per workgroup, one workgroup per CU -- every
//                                    gate still has its two waves, which then share their SIMDs with fewer (or no) other waves
//                                    (or four waves per gate: pair4_tail_gates)
//   a larger remainder             : one more (partly filled) round of 4 gates per CU
//   a last whole round and a remainder of up to rr gates per CU together (rr_applies): ONE launch of five or six gates per CU, (4 + rem / CUs) / 4
//                                    rounds instead of 2 (1,280 gates 9.3 -> 8.2 ms; profiles/r06/pair_rr_sweep.log)
// RTFHE_FORCE_WAVES=1|2|4|8 forces one shape for the whole batch (4, 8: one gate per wave in 4- / 8-wave workgroups).  A programmable
// bootstrap takes the same shapes on the k_pbs_* twins.
int launch_bootstrap_n1024(rtfhe_ctx* ctx, const BootstrapArgs& a, hipStream_t s, const LutRef& lut) {
    const int force = ctx->force_waves;
    if (force == 1) return Wg::launch(ctx, 1, a, s, lut);
    if (force == 2) return Pair::launch(ctx, 4, a, s, lut);
    if (force == 4 || force == 8) return Wave10::launch(ctx, force, a, s, lut);
    return walk_ladder(ctx, a, s, lut, 4, rr_applies(ctx, (size_t)a.count), [&](const BootstrapArgs& b, const LutRef& l, int gates, bool tail) {
        if (!tail) return Pair::launch(ctx, 4, b, s, l);
        if (gates > 4) return PairRr::launch(ctx, gates, b, s, l);
        if ((size_t)b.count <= (size_t)ctx->wg_max) return Wg::launch(ctx, 1, b, s, l);
        const bool p4 = ctx->p4bk_valid && (b.mode == MODE_EXTRACT || b.mode == MODE_BLIND_ROTATE);      // (a split MODE_GATE batch comes here in MODE_EXTRACT)
        if (const int g4 = p4 ? pair4_tail_gates(ctx, (size_t)b.count) : 0) return Pair4::launch(ctx, g4, b, s, l);
        return Pair::launch(ctx, gates < 2 ? 2 : gates, b, s, l);
    });
}

// N = 2048: two waves per transform (two waves per SIMD, no AGPR traffic) in whole rounds of eo_round gates per CU and a tail.  Up to two gates per
// CU: four waves per gate, so that no SIMD is left with a lone wave (single gate 9.78 -> 5.84 ms, 512 gates 9.91 -> 7.8 ms,
// profiles/r04/n2048_four_waves_per_gate_ab.log); the fused key switch stays on the two-wave kernels.  Without the tables or the key layout of
// those kernels, and under RTFHE_FORCE_WAVES=4: one wave per gate (inverse pass-1/untwist twiddles in global memory: 4 gates per CU fit).
int launch_bootstrap_n2048(rtfhe_ctx* ctx, const BootstrapArgs& a, hipStream_t s, const LutRef& lut) {
    if (!(ctx->d_etw && ctx->ebk_valid) || ctx->force_waves == 4) return Wave11::launch(ctx, 4, a, s, lut);
    return walk_ladder(ctx, a, s, lut, ctx->eo_round, false, [&](const BootstrapArgs& b, const LutRef& l, int gates, bool) {
        const bool four = gates <= 2 && ctx->eo4 && (b.mode == MODE_EXTRACT || b.mode == MODE_BLIND_ROTATE);
        return four ? Eo4::launch(ctx, gates, b, s, l) : Eo::launch(ctx, gates, b, s, l);
    });
}

// Every (kernel family, gates per workgroup) the dispatch above can launch fits the CU's LDS at the longest mask the context accepts
// (NPAD_MAX); where a family takes fewer gates at long masks, the function that prime_fft_kernels decides with is the one checked here.
static_assert(Pair::fits(NPAD_MAX) && Wg::fits(NPAD_MAX) && Pair4::fits(NPAD_MAX) && Wave10::fits(NPAD_MAX) && Wave11::fits(NPAD_MAX) && Eo4::fits(NPAD_MAX), "every shape at every mask length");
static_assert(rr_fit<PairRrLds>(640) == 6 && rr_fit<PairRrLds>(704) == 5 && rr_fit<PairRrLds>(NPAD_MAX) == 5, "k_bootstrap_pair_rr: six gates per CU up to n = 639, five beyond");
static_assert(PairRr::fits(NPAD_MAX, rr_fit<PairRrLds>(NPAD_MAX)), "k_bootstrap_pair_rr at the longest mask");
static_assert(eo_round_gates(704) == 4 && eo_round_gates(NPAD_MAX) == 3, "k_bootstrap_eo: four gates per CU up to n = 703, three beyond");
static_assert(Eo::fits(NPAD_MAX, eo_round_gates(NPAD_MAX)), "k_bootstrap_eo at the longest mask");

// which second key layout the dispatch above reads for a batch of `count` gates in `mode` (0 = none)
enum { LAYOUT_NONE = 0, LAYOUT_P4 = 1, LAYOUT_EO = 2 };
int layout_needed(const rtfhe_ctx* ctx, size_t count, int mode) {
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR) return LAYOUT_NONE;
    if (ctx->logn == 11) return ctx->force_waves == 4 ? LAYOUT_NONE : LAYOUT_EO;
    if (ctx->force_waves) return LAYOUT_NONE;
    if (rr_applies(ctx, count)) return LAYOUT_NONE;      // the remainder rides with the last whole round (k_bootstrap_pair_rr reads d_bk)
    // (a MODE_GATE batch reaches the four-wave kernel through the split path only, as MODE_EXTRACT: without the matrix form of the key it stays on the fused
    // kernels.  This runs before the stream's scratch exists, so it cannot ask split_ok: it restates the part of it that is known by now.)
    if (mode == MODE_GATE && !(ctx->d_ksmat && ctx->ks_mm_min > 0 && count >= (size_t)ctx->ks_mm_min)) return LAYOUT_NONE;
    return pair4_tail_gates(ctx, count % ((size_t)4 * ctx->num_cus)) ? LAYOUT_P4 : LAYOUT_NONE;
}

}  // namespace

// ---- the device tables of the kernel families of this unit (HostTw: rtfhe_host.hpp, rtfhe_twiddles.hip) ----
// table of k_bootstrap_eo (N = 2048; layout: EoTw): wave H owns the points i = 2 j + H and runs nine of the ten stages on the 512-point
// sub-sequence j; the twiddle of pair (i, i + halfnn) is entry i mod halfnn = 2 (j mod halfnn / 2) + H of the reference's stage table
std::vector<cplx> HostTw::eo_table() const {
    typedef Geo<10> G;
    std::vector<cplx> t(EoTw::TOTAL, make_double2(0.0, 0.0));
    const double fold = 2.0 / (double)N;      // the inverse's input scaling (fft_processor_spqlios.cpp:158), exact, folded into the untwist
    for (int H = 0; H < 2; H++) {
        for (int m = 0; m < 8; m++)
            for (int lane = 0; lane < 64; lane++) {
                const int i = 2 * (lane + 64 * m) + H;
                t[EoTw::TWIST + (H * 8 + m) * 64 + lane] = make_double2(twist_c[i], twist_s[i]);
                t[EoTw::IUNTW + (H * 8 + m) * 64 + lane] = make_double2(untw_c[i] * fold, untw_s[i] * fold);
            }
        for (int mb = G::LR - 1; mb >= 0; mb--) {
            const int h = 1 << mb;
            for (int q = 0; q < h; q++) {
                const int e = G::R - 2 * h + q;
                for (int lane = 0; lane < 64; lane++) {           // pass 1: j-halfnn 64 h = i-halfnn 128 h
                    const int k = 2 * (lane + 64 * q) + H;
                    t[EoTw::P1 + (H * 7 + e) * 64 + lane] = make_double2(fwd_c[fwd_off(128 * h) + k], fwd_s[fwd_off(128 * h) + k]);
                    t[EoTw::IP1 + (H * 7 + e) * 64 + lane] = make_double2(inv_c[inv_off(128 * h) + k], inv_s[inv_off(128 * h) + k]);
                }
                for (int r = 0; r < G::NLOW; r++) {               // pass 2: j-halfnn 8 h = i-halfnn 16 h
                    const int k = 2 * ((q << G::LOW) | r) + H;
                    t[EoTw::P2 + (H * 7 + e) * G::NLOW + r] = make_double2(fwd_c[fwd_off(16 * h) + k], fwd_s[fwd_off(16 * h) + k]);
                    t[EoTw::IP2 + (H * 7 + e) * G::NLOW + r] = make_double2(inv_c[inv_off(16 * h) + k], inv_s[inv_off(16 * h) + k]);
                }
            }
        }
        for (int q = 0; q < 4; q++) {                             // pass 3: i-halfnn 8 (entries 0..3) and 4 (entries 4..5)
            t[EoTw::P3 + H * 8 + q] = make_double2(fwd_c[fwd_off(8) + 2 * q + H], fwd_s[fwd_off(8) + 2 * q + H]);
            t[EoTw::IP3 + H * 8 + q] = make_double2(inv_c[inv_off(8) + 2 * q + H], inv_s[inv_off(8) + 2 * q + H]);
        }
        for (int q = 0; q < 2; q++) {
            t[EoTw::P3 + H * 8 + 4 + q] = make_double2(fwd_c[fwd_off(4) + 2 * q + H], fwd_s[fwd_off(4) + 2 * q + H]);
            t[EoTw::IP3 + H * 8 + 4 + q] = make_double2(inv_c[inv_off(4) + 2 * q + H], inv_s[inv_off(4) + 2 * q + H]);
        }
    }
    return t;
}

// tables of the parity sub-networks of the latency kernel (N = 1024; layout: Q4Tw, rtfhe_sub256.hpp): wave H owns the points i = 2 j + H of a
// 512-point transform and runs its twiddled stages on the 256-point sub-sequence j; the twiddle of pair (i, i + halfnn) is entry
// i mod halfnn = 2 (j mod halfnn / 2) + H of the reference's stage table
std::vector<cplx> HostTw::q4_table() const {
    std::vector<cplx> t(Q4Tw::TOTAL, make_double2(0.0, 0.0));
    const double fold = 2.0 / (double)N;      // the inverse's input scaling (fft_processor_spqlios.cpp:158), exact, folded into the untwist
    for (int dir = 0; dir < 2; dir++)
        for (int H = 0; H < 2; H++) {
            cplx* d = t.data() + Q4Tw::off(dir, H);
            const double* sc = dir ? inv_c.data() : fwd_c.data();
            const double* ss = dir ? inv_s.data() : fwd_s.data();
            auto off = [&](int halfnn) { return dir ? inv_off(halfnn) : fwd_off(halfnn); };
            auto entry = [&](int halfnn, int k) { return make_double2(sc[off(halfnn) + k], ss[off(halfnn) + k]); };
            for (int m = 0; m < 4; m++)
                for (int lane = 0; lane < 64; lane++) {
                    const int i = 2 * (lane + 64 * m) + H;
                    d[Q4Tw::TW + m * 64 + lane] = dir ? make_double2(untw_c[i] * fold, untw_s[i] * fold) : make_double2(twist_c[i], twist_s[i]);
                }
            for (int mb = 1; mb >= 0; mb--) {
                const int h = 1 << mb;
                for (int q = 0; q < h; q++) {
                    const int e = 4 - 2 * h + q;
                    for (int lane = 0; lane < 64; lane++) d[Q4Tw::P1 + e * 64 + lane] = entry(128 * h, 2 * (lane + 64 * q) + H);     // pass 1: j-halfnn 64 h
                    for (int r = 0; r < 16; r++) d[Q4Tw::P2 + e * 16 + r] = entry(32 * h, 2 * ((q << 4) | r) + H);                  // pass 2: j-halfnn 16 h
                    for (int c = 0; c < 4; c++) d[Q4Tw::P3 + e * 4 + c] = entry(8 * h, 2 * ((q << 2) | c) + H);                     // pass 3: j-halfnn 4 h
                }
            }
            for (int q = 0; q < 2; q++) d[Q4Tw::P4 + q] = entry(4, 2 * q + H);                                                      // pass 4: i-halfnn 4
        }
    return t;
}

namespace rtfhe_host {

int launch_bootstrap_fft(rtfhe_ctx* ctx, BootstrapArgs a, hipStream_t s, const LutRef& lut) {
    return ctx->logn == 10 ? launch_bootstrap_n1024(ctx, a, s, lut) : launch_bootstrap_n2048(ctx, a, s, lut);
}

// The key spectra once more in the layout a kernel family reads (derived from d_bk on this context's device), built by the first batch whose
// dispatch needs it -- a context that never runs such a batch never pays for the copy (N = 2048: 125 MB, N = 1024: 62 MB).  Called outside
// stream captures only (it allocates and synchronises); a dispatch inside a capture that finds the layout absent takes the kernels that read d_bk.
static int build_bk_layout(rtfhe_ctx* ctx, int which) {
    cplx** dst = which == LAYOUT_EO ? &ctx->d_ebk : &ctx->d_p4bk;
    bool* valid = which == LAYOUT_EO ? &ctx->ebk_valid : &ctx->p4bk_valid;
    const size_t polys = bk_word_count(ctx->p) / ctx->p.N;
    if (!*dst) HIPCHECK(ctx, hipMalloc((void**)dst, bk_cplx_count(ctx->p) * sizeof(cplx)));
    // (three scalar arguments, not one struct: launched by hand, not counted)
    if (which == LAYOUT_EO) hipLaunchKernelGGL(k_bk_to_eo, dim3(2048), dim3(256), 0, ctx->stream, (const cplx*)ctx->d_bk, *dst, polys);
    else hipLaunchKernelGGL(k_bk_to_p4, dim3(2048), dim3(256), 0, ctx->stream, (const cplx*)ctx->d_bk, *dst, polys);
    HIPCHECK(ctx, hipGetLastError());
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    *valid = true;
    return 0;
}

int ensure_bk_layouts(rtfhe_ctx* ctx, size_t count, int mode) {
    const int need = layout_needed(ctx, count, mode);
    if (need == LAYOUT_NONE || !ctx->d_bk) return 0;
    if (need == LAYOUT_EO ? ctx->ebk_valid : ctx->p4bk_valid) return 0;
    return build_bk_layout(ctx, need);
}

// A new key has just been put into d_bk (and d_bk_torus): every derived form of the key whose BUFFER ALREADY EXISTS is rebuilt in place, now,
// synchronously.  Such a buffer's address may be baked into a HIP graph -- one of this context's circuits, or a capture the caller took around a
// *_dev call -- and a replay must find the new key there, not the old key's spectra until some later eager batch happens to rebuild them
// (advisor r5).  Forms that were never built stay unbuilt (built on demand, ensure_bk_layouts / ntt_prepare / xfft_prepare).  The exact backends'
// forms derive from the torus form of the key: a key that came as spectra (rtfhe_load_bk_fft) has none, the old forms cannot be rebuilt, and
// the circuits recorded on those backends are marked stale (rtfhe_circuit_launch then fails with RTFHE_ERR_STATE instead of computing with
// the old key).
int rebuild_derived_keys(rtfhe_ctx* ctx) {
    if (int rc = use(ctx)) return rc;
    if (ctx->d_ebk) if (int rc = build_bk_layout(ctx, LAYOUT_EO)) return rc;
    if (ctx->d_p4bk) if (int rc = build_bk_layout(ctx, LAYOUT_P4)) return rc;
    if (ctx->d_bk_torus) {
        if (ctx->d_ntt_bk) if (int rc = ntt_prepare(ctx)) return rc;
        if (ctx->d_xbk) if (int rc = xfft_prepare(ctx)) return rc;
    } else if (ctx->d_ntt_bk || ctx->d_xbk) {
        for (rtfhe_circuit* c : ctx->circuits)
            if (c->backend != RTFHE_BACKEND_FFT64_MIRROR) c->stale = true;
    }
    return 0;
}

// grants every bootstrap kernel of this context's parameter set, and its twins, its dynamic LDS once, at context creation: the families the
// dispatch above launches from, each at the gate counts its Family lists
int prime_fft_kernels(rtfhe_ctx* ctx) {
    const int npad = (ctx->p.n + 1 + 63) / 64 * 64;
    if (ctx->logn == 10) {
        if (int rc = Pair::prime(ctx, npad)) return rc;
        if (int rc = Wg::prime(ctx, npad)) return rc;
        // the time-sliced launch: as many gates per CU (five or six) as this mask length leaves room for in 160 KiB of LDS
        ctx->rr = std::min(ctx->rr, rr_fit<PairRrLds>(npad));
        if (int rc = PairRr::prime(ctx, npad, ctx->rr)) return rc;
        if (int rc = Pair4::prime(ctx, npad)) return rc;
        return Wave10::prime(ctx, npad);
    }
    if (int rc = Wave11::prime(ctx, npad)) return rc;
    // whole rounds of four gates per CU where their LDS fits, of three at the longest masks (the four-gate kernel is then never launched)
    ctx->eo_round = eo_round_gates(npad);
    if (int rc = Eo::prime(ctx, npad, ctx->eo_round)) return rc;
    return Eo4::prime(ctx, npad);
}

}  // namespace rtfhe_host
