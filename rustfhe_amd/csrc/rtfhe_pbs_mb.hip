// rtfhe_pbs_mb.hip -- multi-bit blind rotation (include/rtfhe.h: rtfhe_mbk_create, rtfhe_pbs_mb_batch[_dev]): multi-bit keys -- the TRGSW samples of
// every group of g key bits as spectra, converted as a selector set's are, with the roots table and the point map of the key combination beside
// them --, the argument checks (rtfhe_mb_plan.cpp, host only), the choice between the two kernel shapes and the rules around stream captures.
// One launch of k_pbs_mb or k_pbs_mb_wg (their ROUNDED twins under rtfhe_set_decomposition) runs all ceil(n / g) steps of all gates; behind it
// the extract tail every entry point with lvl1 samples shares (launch_key_switch_rows_restore: where table indices are given, k_rows_restore
// puts back the rows of skipped gates); or the kernel's own key switch.
#include "rtfhe_host.hpp"

#include <cstdlib>
#include <cstring>

#include "rtfhe_kernels_pbs_mb.hpp"
#include "rtfhe_kernels_pbs_mb_wg.hpp"
#include "rtfhe_mb_plan.h"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

typedef void (*MbKernel)(PbsMbArgs);
struct MbShape { MbKernel reference, rounded; size_t lds; int gates_per_wg, threads; };

MbShape wave_shape(const rtfhe_ctx* ctx, int npad) {
    if (ctx->logn == 11) return {k_pbs_mb<11, false>, k_pbs_mb<11, true>, pbs_mb_lds_bytes<11>(npad), MB_WAVES, 64 * MB_WAVES};
    return {k_pbs_mb<10, false>, k_pbs_mb<10, true>, pbs_mb_lds_bytes<10>(npad), MB_WAVES, 64 * MB_WAVES};
}
MbShape wg_shape(int npad) { return {k_pbs_mb_wg<false>, k_pbs_mb_wg<true>, pbs_mb_wg_lds_bytes(npad), 1, 64 * MB_WG_WAVES}; }

int npad_of(const rtfhe_ctx* ctx) { return (ctx->p.n + 1 + 63) / 64 * 64; }

// both twins of both shapes are granted their LDS when a key is made, so that the first call of a context may already sit in a stream capture
int prime_mb(rtfhe_ctx* ctx) {
    const int npad = npad_of(ctx);
    const MbShape w = wave_shape(ctx, npad);
    if (w.lds > LDS_LIMIT) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_mbk_create: n = " + std::to_string(ctx->p.n) + " leaves the multi-bit kernel no room in LDS");
    if (int rc = allow_lds(ctx, w.reference, w.lds)) return rc;
    if (int rc = allow_lds(ctx, w.rounded, w.lds)) return rc;
    if (ctx->logn != 10) return 0;
    const MbShape g = wg_shape(npad);
    if (int rc = allow_lds(ctx, g.reference, g.lds)) return rc;
    return allow_lds(ctx, g.rounded, g.lds);
}

// RTFHE_MB_SHAPE=wave|wg forces one shape (read when the call is made); otherwise N = 1024 takes the workgroup shape and N = 2048 the wave
// shape.  (The rule this began with sent N = 1024 batches of more than one gate per CU to the wave shape; measured, the workgroup shape is
// the faster one at every count up to 1,024 gates -- 15.7 against 22.2 ms there -- and no crossover was found: DESIGN.md 5.24.)
int pick_shape(rtfhe_ctx* ctx, size_t, bool& wg) {
    wg = ctx->logn == 10;
    const char* e = std::getenv("RTFHE_MB_SHAPE");
    if (!e || !*e) return 0;
    if (!std::strcmp(e, "wave")) { wg = false; return 0; }
    if (!std::strcmp(e, "wg")) {
        if (ctx->logn != 10) return fail(ctx, RTFHE_ERR_INVALID, "RTFHE_MB_SHAPE=wg: the workgroup shape exists at N = 1024 only");
        wg = true;
        return 0;
    }
    return fail(ctx, RTFHE_ERR_INVALID, std::string("RTFHE_MB_SHAPE=") + e + ": wave or wg");
}

// what both entries check before anything is allocated or launched; host_idx is null in the _dev form, whose array the kernel checks
int mb_ready(rtfhe_ctx* ctx, const rtfhe_mbk* mbk, const rtfhe_lut* lut, const int32_t* host_idx, const void* tlwe, const void* out, size_t count, bool& wg) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = handles_ready(ctx, {ref(mbk), ref(lut)})) return rc;
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "programmable bootstrapping runs on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); "
                                            "select it with rtfhe_set_backend");
    if (!ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    if (lut->encrypted) return fail(ctx, RTFHE_ERR_INVALID, "the multi-bit PBS takes plain tables (rtfhe_lut_create), not an encrypted one");
    char err[256];
    if (int rc = rtfhe_mb_call_plan(ctx->p.n, mbk->g, count, host_idx, lut->n_lut, tlwe, out, err, sizeof err)) return fail(ctx, rc, err);
    return pick_shape(ctx, count, wg);
}

// `count` gates on device buffers, primary device, stream s.  Inside a stream capture, and in a context without the matrix form of the
// key-switching key (RTFHE_KS_MM_MIN=0), the kernel switches keys itself and nothing is allocated; otherwise the samples go through this
// stream's sample buffer (grown here, outside captures only) into the batch key switch.
int launch_mb(rtfhe_ctx* ctx, const rtfhe_mbk* mbk, const rtfhe_lut* lut, const int32_t* d_idx, const void* d_in, void* d_out, size_t count, bool wg, hipStream_t s) {
    if (count == 0) return 0;
    StreamScratch* samples = nullptr;
    if (!capturing(s) && ctx->d_ksmat && ctx->ks_mm_min > 0)
        if (int rc = stream_scratch(ctx, ctx->tlwe1, s, false, tlwe1_shape(ctx), count, "", samples)) return rc;
    PbsMbArgs a{};
    a.tw = ctx->d_tw; a.mbk = mbk->d_spec; a.roots = mbk->d_roots; a.qmap = mbk->d_qmap; a.ksk = ctx->d_ksk;
    a.in = (const uint32_t*)d_in; a.out = (uint32_t*)d_out; a.ext = samples ? samples->d[0] : nullptr;
    a.tv = lut->d_tv[0]; a.tv_idx = d_idx; a.fault = ctx->d_fault;
    a.n_tv = lut->n_lut; a.count = (int32_t)count; a.n = ctx->p.n; a.g = mbk->g; a.ksw = ctx->ksw; a.npad = npad_of(ctx);
    const MbShape k = wg ? wg_shape(a.npad) : wave_shape(ctx, a.npad);
    const dim3 grid((unsigned)((count + k.gates_per_wg - 1) / k.gates_per_wg)), block(k.threads);
    if (int rc = launch_kernel(ctx, ctx->decomp == RTFHE_DECOMP_ROUNDED ? k.rounded : k.reference, grid, block, k.lds, s, a)) return rc;
    if (!samples) return 0;
    // the key switch has written every row: the rows of skipped gates come back from where their gates parked them (not counted: no gate runs in it)
    return launch_key_switch_rows_restore(ctx, samples->d[0], (uint32_t*)d_out, count, d_idx, 1, lut->n_lut, false, s);
}

}  // namespace

namespace rtfhe_host {

void mbk_release(rtfhe_mbk* k) {
    (void)hipSetDevice(k->ctx->device);
    if (k->d_spec) (void)hipFree(k->d_spec);
    if (k->d_roots) (void)hipFree(k->d_roots);
    if (k->d_qmap) (void)hipFree(k->d_qmap);
    k->d_spec = nullptr; k->d_roots = nullptr; k->d_qmap = nullptr;
}

}  // namespace rtfhe_host

extern "C" {

int rtfhe_mbk_create(rtfhe_ctx* ctx, const uint32_t* words, int32_t g, rtfhe_mbk** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_mbk_create: null argument");
    *out = nullptr;
    char err[256];
    if (int rc = rtfhe_mb_key_plan(ctx->p.n, ctx->p.N, ctx->p.l, g, words, err, sizeof err)) return fail(ctx, rc, std::string("rtfhe_mbk_create: ") + err);
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "programmable bootstrapping runs on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); "
                                            "select it with rtfhe_set_backend");
    if (int rc = use(ctx)) return rc;
    if (int rc = prime_mb(ctx)) return rc;
    const int N = ctx->p.N;
    const int32_t n_trgsw = (int32_t)rtfhe_mb_trgsw_count(ctx->p.n, g);
    const size_t spec_bytes = (size_t)n_trgsw * 2 * 2 * ctx->p.l * (N / 2) * sizeof(cplx), roots_bytes = (size_t)2 * N * sizeof(cplx), qmap_bytes = (size_t)(N / 2) * 4;
    std::vector<double> roots((size_t)4 * N);
    std::vector<int32_t> qmap((size_t)N / 2);
    if (rtfhe_mb_roots(N, roots.data()) || rtfhe_mb_point_exponents(N, qmap.data())) return fail(ctx, RTFHE_ERR_STATE, "rtfhe_mbk_create: tables");
    NewHandle<rtfhe_mbk> k = new_handle(ctx, mbk_release);
    k->g = g; k->n_trgsw = n_trgsw; k->bytes = spec_bytes + roots_bytes + qmap_bytes;
    int rc = 0;
    if (hipMalloc((void**)&k->d_spec, spec_bytes) != hipSuccess || hipMalloc((void**)&k->d_roots, roots_bytes) != hipSuccess ||
        hipMalloc((void**)&k->d_qmap, qmap_bytes) != hipSuccess)
        rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_mbk_create: hipMalloc");
    if (!rc && (hipMemcpy(k->d_roots, roots.data(), roots_bytes, hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(k->d_qmap, qmap.data(), qmap_bytes, hipMemcpyHostToDevice) != hipSuccess))
        rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_mbk_create: hipMemcpy (tables)");
    // the words become spectra as a selector set's do (TRGSWRepF::from of every sample)
    if (!rc) rc = convert_selectors(ctx, k->d_spec, n_trgsw, [&](size_t nwords) { return copy_in(ctx, ctx->d_a, words, nwords * 4, 0); });
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_mbk_create: hipStreamSynchronize");
    return rc ? rc : handle_publish(ctx->mbks, std::move(k), out);
}

void rtfhe_mbk_destroy(rtfhe_mbk* k) { handle_destroy(&rtfhe_ctx::mbks, k, mbk_release); }

int rtfhe_pbs_mb_batch(rtfhe_ctx* ctx, const rtfhe_mbk* mbk, const rtfhe_lut* lut, const int32_t* lut_idx, const uint32_t* tlwe, uint32_t* out, size_t count) {
    bool wg = false;
    if (int rc = mb_ready(ctx, mbk, lut, lut_idx, tlwe, out, count, wg)) return rc;
    // host buffers: the rows ride in d_a, lut_idx in d_b, the result comes back through d_c
    const size_t bytes = count * ((size_t)ctx->p.n + 1) * 4;
    return host_form(ctx, count, {staging_a(ctx), tlwe, bytes}, {staging_c(ctx), out, bytes, false}, {{staging_b(ctx), count, lut_idx, nullptr}},
                     [&](const void* d_tlwe, const StagedIdx* idx, void* d_out) { return launch_mb(ctx, mbk, lut, idx[0].first, d_tlwe, d_out, count, wg, ctx->stream); });
}

int rtfhe_pbs_mb_batch_dev(rtfhe_ctx* ctx, const rtfhe_mbk* mbk, const rtfhe_lut* lut, const void* d_lut_idx, const void* d_tlwe, void* d_out, size_t count,
                           void* stream) {
    bool wg = false;
    if (int rc = mb_ready(ctx, mbk, lut, nullptr, d_tlwe, d_out, count, wg)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, "rtfhe_pbs_mb_batch_dev", {d_tlwe, d_out}, {d_lut_idx})) return rc;
    return launch_mb(ctx, mbk, lut, (const int32_t*)d_lut_idx, d_tlwe, d_out, count, wg, (hipStream_t)stream);
}

}  // extern "C"
