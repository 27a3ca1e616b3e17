// rtfhe_dense.hip -- lvl0 dense layers (include/rtfhe.h: rtfhe_dense_create, rtfhe_tlwe_dense_batch[_dev]): a layer holds an integer matrix as
// signed bytes in the i8 matrix pipe's operand order and its per-output correction words; a call multiplies it into a batch of TLWE rows, every
// word exact mod 2^32 (rtfhe_kernels_dense.hpp).  No key is read and no backend is asked: the calls work on every backend.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_dense.hpp"
#include "rtfhe_dense_plan.h"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// what every entry checks before anything is allocated or launched: the handles, then the arguments themselves (rtfhe_dense_plan, host only)
int dense_ready(rtfhe_ctx* ctx, const rtfhe_dense* w, const void* x, const void* out, size_t count) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = handles_ready(ctx, {ref(w)})) return rc;
    char err[256];
    if (int rc = rtfhe_dense_plan(ctx->p.n, w->O, w->I, count, x, out, err, sizeof err)) return fail(ctx, rc, err);
    return 0;
}

// `count` samples on device buffers, primary device, stream s; nothing allocated.  Without a bias ONE launch; with one, one launch per
// DENSE_BIAS_MAX outputs (the bias words ride in the launch's arguments: the caller's host array is read now, never by the device).  The launch
// rule is asked per launch, with that launch's outputs, so the launches of one call may take different paths (a last, small one cut into slices
// behind whole ones with plain stores).  The clearing is therefore decided ONCE, before the first launch: where any launch of a call that does
// not accumulate cuts I into slices, the whole output is cleared first (a memset node, no kernel) -- never between two launches, where it would
// wipe what an earlier one stored.
int launch_dense(rtfhe_ctx* ctx, const rtfhe_dense* w, const void* d_x, const uint32_t* bias, int32_t accumulate, void* d_out, size_t count, hipStream_t s) {
    if (count == 0) return 0;
    const int32_t n = ctx->p.n, chunk = bias ? DENSE_BIAS_MAX : w->O;
    const auto shape_of = [&](int32_t o_first) {
        rtfhe_dense_shape sh;
        rtfhe_dense_launch_shape(n, std::min(w->O, o_first + chunk) - o_first, w->I, count, ctx->num_cus, &sh);
        return sh;
    };
    if (!accumulate) {
        bool sliced = false;
        for (int32_t o_first = 0; o_first < w->O; o_first += chunk) sliced = sliced || shape_of(o_first).slices > 1;
        if (sliced) HIPCHECK(ctx, hipMemsetAsync(d_out, 0, count * (size_t)w->O * ((size_t)n + 1) * 4, s));
    }
    for (int32_t o_first = 0; o_first < w->O; o_first += chunk) {
        DenseArgs a{};
        a.wmat = w->d_wmat; a.corr = w->d_corr; a.x = (const uint32_t*)d_x; a.out = (uint32_t*)d_out;
        a.count = (int32_t)count; a.O = w->O; a.I = w->I; a.n = n;
        a.o_first = o_first; a.o_end = std::min(w->O, o_first + chunk);
        const rtfhe_dense_shape sh = shape_of(o_first);
        a.groups = sh.groups; a.cwgs = sh.cwgs; a.ksteps = sh.ksteps; a.slices = sh.slices; a.steps = sh.steps;
        a.accumulate = accumulate ? 1 : 0; a.has_bias = bias ? 1 : 0;
        if (bias) std::memcpy(a.bias, bias + o_first, (size_t)(a.o_end - a.o_first) * 4);
        a.total = (uint32_t)(count * (size_t)sh.cwgs * (size_t)sh.slices * (size_t)sh.groups);
        const unsigned grid = (unsigned)((std::min<size_t>(a.total, (size_t)1 << 20) + 7) / 8 * 8);
        int rc = sh.tiles == 4 ? launch_kernel(ctx, k_tlwe_dense<4>, dim3(grid), dim3(64 * DENSE_WAVES), 0, s, a)
               : sh.tiles == 2 ? launch_kernel(ctx, k_tlwe_dense<2>, dim3(grid), dim3(64 * DENSE_WAVES), 0, s, a)
                               : launch_kernel(ctx, k_tlwe_dense<1>, dim3(grid), dim3(64 * DENSE_WAVES), 0, s, a);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

namespace rtfhe_host {

void dense_release(rtfhe_dense* w) {
    (void)hipSetDevice(w->ctx->device);
    if (w->d_wmat) (void)hipFree(w->d_wmat);
    if (w->d_corr) (void)hipFree(w->d_corr);
    w->d_wmat = nullptr; w->d_corr = nullptr;
}

}  // namespace rtfhe_host

extern "C" {

int rtfhe_dense_create(rtfhe_ctx* ctx, const int32_t* W, int32_t O, int32_t I, rtfhe_dense** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_dense_create: null argument");
    *out = nullptr;
    char err[256];
    std::vector<uint32_t> corr(O >= 1 && O <= RTFHE_DENSE_MAX ? (size_t)O : 1);
    if (int rc = rtfhe_dense_weights_plan(W, O, I, corr.data(), err, sizeof err)) return fail(ctx, rc, std::string("rtfhe_dense_create: ") + err);
    if (int rc = use(ctx)) return rc;
    // the three kernel shapes are noted as granted (no dynamic LDS: nothing is called in HIP), so that a first call may sit in a stream capture
    if (int rc = allow_lds(ctx, k_tlwe_dense<1>, 0)) return rc;
    if (int rc = allow_lds(ctx, k_tlwe_dense<2>, 0)) return rc;
    if (int rc = allow_lds(ctx, k_tlwe_dense<4>, 0)) return rc;
    NewHandle<rtfhe_dense> t = new_handle(ctx, dense_release);
    t->O = O; t->I = I; t->ksteps = (I + 63) / 64; t->otiles = (O + 15) / 16;
    const size_t raw_bytes = (size_t)O * (size_t)I * 4, mat_v4 = (size_t)t->otiles * (size_t)t->ksteps * 64;
    int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, raw_bytes);
    if (!rc && hipMalloc((void**)&t->d_wmat, mat_v4 * sizeof(uint4)) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_dense_create: hipMalloc");
    if (!rc && hipMalloc((void**)&t->d_corr, (size_t)O * 4) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_dense_create: hipMalloc");
    if (!rc) rc = copy_in(ctx, ctx->d_a, W, raw_bytes, 0);      // on the stream of the build below, which is waited for
    if (!rc && hipMemcpyAsync(t->d_corr, corr.data(), (size_t)O * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_dense_create: hipMemcpyAsync");
    if (!rc) {
        const DenseBuildArgs a{(const int32_t*)ctx->d_a, t->d_wmat, O, I, t->ksteps, t->otiles};
        rc = launch_kernel(ctx, k_dense_build, dim3((unsigned)std::min<size_t>((mat_v4 + 255) / 256, 2048)), dim3(256), 0, ctx->stream, a, false);
    }
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_dense_create: hipStreamSynchronize");
    return rc ? rc : handle_publish(ctx->denses, std::move(t), out);
}

void rtfhe_dense_destroy(rtfhe_dense* w) { handle_destroy(&rtfhe_ctx::denses, w, dense_release); }

// host buffers: the rows ride in d_a, the result comes back through d_c (which takes the caller's out first when accumulating)
int rtfhe_tlwe_dense_batch(rtfhe_ctx* ctx, const rtfhe_dense* w, const uint32_t* x, const uint32_t* bias, int32_t accumulate, uint32_t* out, size_t count) {
    if (int rc = dense_ready(ctx, w, x, out, count)) return rc;
    const size_t row = ((size_t)ctx->p.n + 1) * 4;
    return host_form(ctx, count, {staging_a(ctx), x, count * (size_t)w->I * row}, {staging_c(ctx), out, count * (size_t)w->O * row, accumulate != 0}, {},
                     [&](const void* d_x, const StagedIdx*, void* d_out) { return launch_dense(ctx, w, d_x, bias, accumulate, d_out, count, ctx->stream); });
}

int rtfhe_tlwe_dense_batch_dev(rtfhe_ctx* ctx, const rtfhe_dense* w, const void* d_x, const uint32_t* bias, int32_t accumulate, void* d_out, size_t count,
                               void* stream) {
    if (int rc = dense_ready(ctx, w, d_x, d_out, count)) return rc;
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, "rtfhe_tlwe_dense_batch_dev", {d_out, d_x})) return rc;
    return launch_dense(ctx, w, d_x, bias, accumulate, d_out, count, (hipStream_t)stream);
}

}  // extern "C"
