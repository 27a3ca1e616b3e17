// rtfhe_trlwe_auto.hip -- TRLWE key switching (include/rtfhe.h: rtfhe_trlwe_ksk_create, rtfhe_trlwe_auto_batch[_dev]): switching keys (the
// rows u32[n_t][l][2][N] as spectra on the primary device, through the forward transform rtfhe_trgsw_create converts selectors with) and the
// call that runs a host program of up to 16 automorphism / re-keying steps on every row of a batch in ONE launch of k_trlwe_auto
// (rtfhe_kernels_trlwe_auto.hpp): the FP64 mirror backend only, in the leveled decomposition in force when the call is made, and no key of the
// context.  Its argument checks: rtfhe_trlwe_auto_plan.cpp, host only.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_trlwe_auto.hpp"
#include "rtfhe_trlwe_auto_plan.h"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

static_assert(TRLWE_AUTO_MAX_STEPS == RTFHE_TRLWE_AUTO_MAX_STEPS, "the kernel and the host checks agree on the most steps");

// the family's twins, four waves (= rows) per workgroup at both N, on k_cmux_tree's LDS carve
RTFHE_LEVELED_FAMILY(auto_twins, TrlweAutoArgs, k_trlwe_auto, cmux_tree_lds_bytes<LOGN, LEVELED_WAVES>())

// what both entries check before anything is allocated or launched: the handle, the backend, then the arguments themselves
// (rtfhe_trlwe_auto_plan, host only)
int auto_ready(rtfhe_ctx* ctx, const rtfhe_trlwe_ksk* key, const int32_t* entry, const int32_t* add, int32_t n_steps, const void* x, const void* out, size_t count) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = handles_ready(ctx, {ref(key)})) return rc;
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "the TRLWE key switch runs on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); select it with rtfhe_set_backend");
    char err[256];
    if (int rc = rtfhe_trlwe_auto_plan(ctx->p.N, key->n_t, entry, add, n_steps, count, x, out, err, sizeof err)) return fail(ctx, rc, err);
    return 0;
}

// `count` rows on device buffers, primary device, stream s: ONE launch, nothing allocated.  The program rides in the launch's arguments.
int launch_auto(rtfhe_ctx* ctx, const rtfhe_trlwe_ksk* key, const int32_t* entry, const int32_t* add, int32_t n_steps, const void* d_x, void* d_out, size_t count,
                hipStream_t s) {
    if (count == 0) return 0;
    TrlweAutoArgs a{};
    a.tw = ctx->d_tw; a.key = key->d_spec; a.in = (const uint32_t*)d_x; a.out = (uint32_t*)d_out;
    a.count = (int32_t)count; a.n_steps = n_steps;
    for (int k = 0; k < n_steps; k++) {
        a.entry[k] = entry[k];
        a.tinv[k] = key->tinv[entry[k]];
        if (add && add[k]) a.add |= 1u << k;
    }
    return launch_leveled(ctx, auto_twins(ctx), count, s, a);
}

}  // namespace

namespace rtfhe_host {

void trlwe_ksk_release(rtfhe_trlwe_ksk* k) {
    (void)hipSetDevice(k->ctx->device);
    if (k->d_spec) (void)hipFree(k->d_spec);
    k->d_spec = nullptr;
}

}  // namespace rtfhe_host

extern "C" {

int rtfhe_trlwe_ksk_create(rtfhe_ctx* ctx, const uint32_t* words, const int32_t* t, int32_t n_t, rtfhe_trlwe_ksk** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!words || !out) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trlwe_ksk_create: null argument");
    *out = nullptr;
    char err[256];
    if (int rc = rtfhe_trlwe_auto_exponents_plan(ctx->p.N, t, n_t, err, sizeof err)) return fail(ctx, rc, std::string("rtfhe_trlwe_ksk_create: ") + err);
    if (int rc = use(ctx)) return rc;
    // the kernels are granted their dynamic LDS now, so that the first call of a context may already sit in a stream capture
    if (int rc = prime_leveled(ctx, auto_twins(ctx))) return rc;
    const size_t polys = (size_t)n_t * ctx->p.l * 2, bytes = polys * ctx->p.N * 4;
    NewHandle<rtfhe_trlwe_ksk> k = new_handle(ctx, trlwe_ksk_release);
    k->n_t = n_t;
    for (int e = 0; e < n_t; e++) { k->t[e] = t[e]; k->tinv[e] = rtfhe_trlwe_auto_inverse(ctx->p.N, t[e]); }
    int rc = hipMalloc((void**)&k->d_spec, polys * (ctx->p.N / 2) * sizeof(cplx)) == hipSuccess ? 0 : fail(ctx, RTFHE_ERR_HIP, "rtfhe_trlwe_ksk_create: hipMalloc");
    // TRGSWRepF::from (trgsw.rs:68-76) of the rows, as convert_selectors transforms a selector set: the words viewed as signed i32, forward
    // transform, the device layout [R][64] per polynomial; the rows are (b, a) pairs already, so the polynomials keep their order (rows = 1)
    if (!rc) rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, bytes);
    if (!rc) rc = copy_in(ctx, ctx->d_a, words, bytes, 0);
    if (!rc) rc = launch_fft(ctx, true, FftArgs{ctx->d_tw, ctx->d_a, k->d_spec, (int32_t)polys, 1, 1, 0}, ctx->stream);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_trlwe_ksk_create: hipStreamSynchronize");
    return rc ? rc : handle_publish(ctx->trlwe_ksks, std::move(k), out);
}

void rtfhe_trlwe_ksk_destroy(rtfhe_trlwe_ksk* k) { handle_destroy(&rtfhe_ctx::trlwe_ksks, k, trlwe_ksk_release); }

// host buffers: the rows ride in d_b, the result comes back through d_c
int rtfhe_trlwe_auto_batch(rtfhe_ctx* ctx, const rtfhe_trlwe_ksk* key, const int32_t* entry, const int32_t* add, int32_t n_steps, const uint32_t* x, uint32_t* out,
                           size_t count) {
    if (int rc = auto_ready(ctx, key, entry, add, n_steps, x, out, count)) return rc;
    const size_t bytes = count * 2 * (size_t)ctx->p.N * 4;
    return host_form(ctx, count, {staging_b(ctx), x, bytes}, {staging_c(ctx), out, bytes, false}, {}, [&](const void* d_x, const StagedIdx*, void* d_out) {
        return launch_auto(ctx, key, entry, add, n_steps, d_x, d_out, count, ctx->stream);
    });
}

int rtfhe_trlwe_auto_batch_dev(rtfhe_ctx* ctx, const rtfhe_trlwe_ksk* key, const int32_t* entry, const int32_t* add, int32_t n_steps, const void* d_x, void* d_out,
                               size_t count, void* stream) {
    if (int rc = auto_ready(ctx, key, entry, add, n_steps, d_x, d_out, count)) return rc;
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, "rtfhe_trlwe_auto_batch_dev", {d_out, d_x})) return rc;
    return launch_auto(ctx, key, entry, add, n_steps, d_x, d_out, count, (hipStream_t)stream);
}

}  // extern "C"
