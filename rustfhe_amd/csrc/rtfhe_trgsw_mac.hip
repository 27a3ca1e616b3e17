// rtfhe_trgsw_mac.hip -- TRLWE x TRGSW multiply-accumulate (include/rtfhe.h: rtfhe_trlwe_mul_trgsw_batch[_dev]): up to eight external products
// S[s_idx] (.) x[x_idx] per sample, summed in the frequency domain into a TRLWE row, optionally on top of what the row held.  The selector sets
// are rtfhe_cmux_tree.hip's (rtfhe_trgsw_create, which also grants these kernels their LDS), the arithmetic is the leveled mode's
// (rtfhe_kernels_trgsw_mac.hpp): the FP64 mirror backend only, in the leveled decomposition in force when the call is made, and no key at all.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_trgsw_mac.hpp"
#include "rtfhe_trgsw_mac_plan.h"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

static_assert(TRGSW_MAC_K_MAX == RTFHE_TRGSW_MAC_K_MAX, "the kernels and the host checks agree on the most terms");

// the family's twins, four waves (= samples) per workgroup at both N, on k_cmux_tree's LDS carve
RTFHE_LEVELED_FAMILY(mac_twins, TrgswMacArgs, k_trlwe_mul_trgsw, cmux_tree_lds_bytes<LOGN, LEVELED_WAVES>())

// what both entries check before anything is allocated or launched: the handle, the caller's pointers and the backend (selector_set_ready), then
// the arguments themselves (rtfhe_trgsw_mac_plan, host only).  host_*: the host-side index arrays (null in the _dev form, whose arrays the kernel checks)
int mac_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, bool s_idx_given, const int32_t* host_s_idx, const void* x, int32_t n_x, bool x_idx_given,
              const int32_t* host_x_idx, int32_t K, const void* out, size_t count) {
    if (int rc = selector_set_ready(ctx, sel, false, nullptr, x && out, "the TRLWE x TRGSW product runs")) return rc;
    char err[256];
    if (int rc = rtfhe_trgsw_mac_plan(ctx->p.N, sel->n_sel, K, s_idx_given, host_s_idx, n_x, x_idx_given, host_x_idx, count, x, out, err, sizeof err))
        return fail(ctx, rc, err);
    return 0;
}

// `count` samples on device buffers, primary device, stream s: ONE launch, nothing allocated
int launch_mac(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* d_s_idx, const void* d_x, int32_t n_x, const int32_t* d_x_idx, int32_t K, int accumulate,
               void* d_out, size_t count, hipStream_t s) {
    if (count == 0) return 0;
    TrgswMacArgs a{};
    a.tw = ctx->d_tw; a.sel = sel->d_spec; a.s_idx = d_s_idx; a.x = (const uint32_t*)d_x; a.x_idx = d_x_idx; a.out = (uint32_t*)d_out;
    a.fault = ctx->d_fault;
    a.count = (int32_t)count; a.K = K; a.n_sel = sel->n_sel; a.n_x = n_x; a.accumulate = accumulate ? 1 : 0;
    return launch_leveled(ctx, mac_twins(ctx), count, s, a);
}

}  // namespace

namespace rtfhe_host {

int prime_trgsw_mac(rtfhe_ctx* ctx) { return prime_leveled(ctx, mac_twins(ctx)); }

}  // namespace rtfhe_host

extern "C" {

// host buffers: the rows ride in d_a, the index arrays in d_b (s_idx, then x_idx), the result comes back through d_c (which takes the caller's out
// first when accumulating)
int rtfhe_trlwe_mul_trgsw_batch(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* s_idx, const uint32_t* x, int32_t n_x, const int32_t* x_idx, int32_t K,
                                int accumulate, uint32_t* out, size_t count) {
    if (int rc = mac_ready(ctx, sel, s_idx != nullptr, s_idx, x, n_x, x_idx != nullptr, x_idx, K, out, count)) return rc;
    const size_t row = 2 * (size_t)ctx->p.N * 4;
    return host_form(ctx, count, {staging_a(ctx), x, (size_t)n_x * row}, {staging_c(ctx), out, count * row, accumulate != 0},
                     {{staging_b(ctx), count * (size_t)K, s_idx, x_idx}}, [&](const void* d_x, const StagedIdx* idx, void* d_out) {
        return launch_mac(ctx, sel, idx[0].first, d_x, n_x, idx[0].second, K, accumulate, d_out, count, ctx->stream);
    });
}

int rtfhe_trlwe_mul_trgsw_batch_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_s_idx, const void* d_x, int32_t n_x, const void* d_x_idx, int32_t K,
                                    int accumulate, void* d_out, size_t count, void* stream) {
    if (int rc = mac_ready(ctx, sel, d_s_idx != nullptr, nullptr, d_x, n_x, d_x_idx != nullptr, nullptr, K, d_out, count)) return rc;
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, "rtfhe_trlwe_mul_trgsw_batch_dev", {d_out, d_x}, {d_s_idx, d_x_idx})) return rc;
    return launch_mac(ctx, sel, (const int32_t*)d_s_idx, d_x, n_x, (const int32_t*)d_x_idx, K, accumulate, d_out, count, (hipStream_t)stream);
}

}  // extern "C"
