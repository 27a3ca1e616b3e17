// rtfhe_plain.hip -- exact TRLWE x plain-polynomial products (include/rtfhe.h: rtfhe_plain_create, rtfhe_trlwe_mul_plain_batch[_dev]): a plain set
// holds integer polynomials as spectra, a call adds up to eight products per sample into a TRLWE row, every word exact mod 2^32.  The arithmetic
// is the split-FFT exact backend's (rtfhe_kernels_plain.hpp) whatever backend the context runs its bootstraps on: the calls work on every
// backend and read no key at all.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_plain.hpp"
#include "rtfhe_plain_plan.h"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

static_assert(PLAIN_K_MAX == RTFHE_PLAIN_K_MAX, "the kernels and the host checks agree on the most terms");

constexpr int BUILD_WAVES = 4;
constexpr size_t XB = (size_t)2 * Geo<10>::XSLOTS * sizeof(double);      // one wave's re + im exchange buffers

template <int LOGN>
constexpr size_t table_bytes() { return (size_t)(LOGN == 11 ? xfft::XTw2::TOTAL : xfft::XTw::TOTAL) * sizeof(cplx); }
template <int LOGN>
constexpr size_t build_lds() { return table_bytes<LOGN>() + BUILD_WAVES * XB; }
// N = 1024: the table and four waves' exchange buffers; N = 2048: the table, two waves' exchange buffers and the trade [2 waves][2 sums][4][64]
template <int LOGN>
constexpr size_t mul_lds() { return LOGN == 11 ? table_bytes<11>() + 2 * XB + (size_t)2 * 2 * 4 * 64 * sizeof(cplx) : table_bytes<10>() + PLAIN_WAVES * XB; }
static_assert(mul_lds<10>() <= LDS_LIMIT && mul_lds<11>() <= LDS_LIMIT && build_lds<11>() <= LDS_LIMIT, "one workgroup's LDS");

// the product kernel is granted its dynamic LDS at rtfhe_plain_create, so that the first call of a context may already sit in a stream capture
int prime_plain(rtfhe_ctx* ctx) {
    return ctx->logn == 11 ? allow_lds(ctx, k_trlwe_mul_plain<11>, mul_lds<11>()) : allow_lds(ctx, k_trlwe_mul_plain<10>, mul_lds<10>());
}

// what every product entry checks before anything is allocated or launched: the handles, then the arguments themselves (rtfhe_plain_plan, host
// only).  host_*: the host-side index arrays (null in the _dev form, whose arrays the kernel checks)
int plain_ready(rtfhe_ctx* ctx, const rtfhe_plain* w, bool w_idx_given, const int32_t* host_w_idx, const void* x, int32_t n_x, bool x_idx_given,
                const int32_t* host_x_idx, int32_t K, const void* out, size_t count) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = handles_ready(ctx, {ref(w)})) return rc;
    char err[256];
    if (int rc = rtfhe_plain_plan(ctx->p.N, w->n_w, w->wmax, K, w_idx_given, host_w_idx, n_x, x_idx_given, host_x_idx, count, x, out, err, sizeof err))
        return fail(ctx, rc, err);
    return 0;
}

// `count` samples on device buffers, primary device, stream s: ONE launch, nothing allocated
int launch_mul_plain(rtfhe_ctx* ctx, const rtfhe_plain* w, const int32_t* d_w_idx, const void* d_x, int32_t n_x, const int32_t* d_x_idx, int32_t K,
                     int32_t accumulate, void* d_out, size_t count, hipStream_t s) {
    if (count == 0) return 0;
    PlainMulArgs a{};
    a.xtw = ctx->d_xtw; a.spec = w->d_spec; a.w_idx = d_w_idx; a.x = (const uint32_t*)d_x; a.x_idx = d_x_idx; a.out = (uint32_t*)d_out;
    a.fault = ctx->d_fault;
    a.count = (int32_t)count; a.K = K; a.n_w = w->n_w; a.n_x = n_x; a.accumulate = accumulate ? 1 : 0;
    if (ctx->logn == 11)       // a workgroup of two waves per (sample, polynomial)
        return launch_kernel(ctx, k_trlwe_mul_plain<11>, dim3((unsigned)(2 * count)), dim3(128), mul_lds<11>(), s, a);
    return launch_kernel(ctx, k_trlwe_mul_plain<10>, dim3((unsigned)((2 * count + PLAIN_WAVES - 1) / PLAIN_WAVES)), dim3(64 * PLAIN_WAVES), mul_lds<10>(), s, a);
}

template <int LOGN>
int launch_build(rtfhe_ctx* ctx, const PlainBuildArgs& a) {
    const size_t items = (size_t)a.count * (LOGN == 11 ? 2 : 1);
    size_t grid = (items + BUILD_WAVES - 1) / BUILD_WAVES; if (grid > 2048) grid = 2048;
    return launch_kernel(ctx, k_plain_build<LOGN, BUILD_WAVES>, dim3((unsigned)grid), dim3(64 * BUILD_WAVES), build_lds<LOGN>(), ctx->stream, a, false);
}

}  // namespace

namespace rtfhe_host {

void plain_release(rtfhe_plain* w) {
    (void)hipSetDevice(w->ctx->device);
    if (w->d_spec) (void)hipFree(w->d_spec);
    w->d_spec = nullptr;
}

}  // namespace rtfhe_host

extern "C" {

int rtfhe_plain_create(rtfhe_ctx* ctx, const int32_t* w, int32_t n_w, rtfhe_plain** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_plain_create: null argument");
    *out = nullptr;
    char err[256];
    int64_t wmax = 0;
    if (int rc = rtfhe_plain_weights_plan(ctx->p.N, w, n_w, &wmax, err, sizeof err)) return fail(ctx, rc, std::string("rtfhe_plain_create: ") + err);
    if (int rc = use(ctx)) return rc;
    if (int rc = xfft_table_ensure(ctx)) return rc;
    if (int rc = prime_plain(ctx)) return rc;
    const size_t words = (size_t)n_w * ctx->p.N;
    NewHandle<rtfhe_plain> t = new_handle(ctx, plain_release);
    t->n_w = n_w; t->wmax = wmax;
    int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, words * 4);
    if (!rc && hipMalloc((void**)&t->d_spec, words / 2 * sizeof(cplx)) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_plain_create: hipMalloc");
    if (!rc) rc = copy_in(ctx, ctx->d_a, w, words * 4, 0);      // on the stream of the build below, which is waited for
    if (!rc) {
        const PlainBuildArgs a{ctx->d_xtw, (const int32_t*)ctx->d_a, t->d_spec, n_w};
        rc = ctx->logn == 11 ? launch_build<11>(ctx, a) : launch_build<10>(ctx, a);
    }
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_plain_create: hipStreamSynchronize");
    return rc ? rc : handle_publish(ctx->plains, std::move(t), out);
}

void rtfhe_plain_destroy(rtfhe_plain* w) { handle_destroy(&rtfhe_ctx::plains, w, plain_release); }

// host buffers: the rows ride in d_a, the index arrays in d_b (w_idx, then x_idx), the result comes back through d_c (which takes the caller's out
// first when accumulating)
int rtfhe_trlwe_mul_plain_batch(rtfhe_ctx* ctx, const rtfhe_plain* w, const int32_t* w_idx, const uint32_t* x, int32_t n_x, const int32_t* x_idx, int32_t K,
                                int32_t accumulate, uint32_t* out, size_t count) {
    if (int rc = plain_ready(ctx, w, w_idx != nullptr, w_idx, x, n_x, x_idx != nullptr, x_idx, K, out, count)) return rc;
    const size_t row = 2 * (size_t)ctx->p.N * 4;
    return host_form(ctx, count, {staging_a(ctx), x, (size_t)n_x * row}, {staging_c(ctx), out, count * row, accumulate != 0},
                     {{staging_b(ctx), count * (size_t)K, w_idx, x_idx}}, [&](const void* d_x, const StagedIdx* idx, void* d_out) {
        return launch_mul_plain(ctx, w, idx[0].first, d_x, n_x, idx[0].second, K, accumulate, d_out, count, ctx->stream);
    });
}

int rtfhe_trlwe_mul_plain_batch_dev(rtfhe_ctx* ctx, const rtfhe_plain* w, const void* d_w_idx, const void* d_x, int32_t n_x, const void* d_x_idx, int32_t K,
                                    int32_t accumulate, void* d_out, size_t count, void* stream) {
    if (int rc = plain_ready(ctx, w, d_w_idx != nullptr, nullptr, d_x, n_x, d_x_idx != nullptr, nullptr, K, d_out, count)) return rc;
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, "rtfhe_trlwe_mul_plain_batch_dev", {d_out, d_x}, {d_w_idx, d_x_idx})) return rc;
    return launch_mul_plain(ctx, w, (const int32_t*)d_w_idx, d_x, n_x, (const int32_t*)d_x_idx, K, accumulate, d_out, count, (hipStream_t)stream);
}

}  // extern "C"
