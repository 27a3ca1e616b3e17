// rtfhe_cmux_net.hip -- CMUX netlists (include/rtfhe.h: rtfhe_cmux_circuit_create, rtfhe_trgsw_update): a decision diagram over
// TRGSW-encrypted inputs, checked and levelised on the host (rtfhe_cmux_net_plan.cpp), recorded once into one linear HIP graph -- the check
// kernel, one launch of k_cmux_net per level (its ROUNDED twin when the leveled mode in force at creation is the rounded one), the output
// kernel, and in the extract form the batch key switch -- and replayed through rtfhe_circuit_launch.
#include "rtfhe_host.hpp"

#include <utility>

#include "rtfhe_cmux_net_plan.h"
#include "rtfhe_kernels_cmux_net.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

constexpr int NET_WAVES = 4;      // four waves (= nodes) per workgroup at both N, the tree's shape

template <int LOGN>
int prime_net_t(rtfhe_ctx* ctx) {
    if (int rc = allow_lds(ctx, k_cmux_net<LOGN, 3, 6, NET_WAVES, false>, cmux_tree_lds_bytes<LOGN, NET_WAVES>())) return rc;
    return allow_lds(ctx, k_cmux_net<LOGN, 3, 6, NET_WAVES, true>, cmux_tree_lds_bytes<LOGN, NET_WAVES>());
}

unsigned blocks_of(size_t waves) { return (unsigned)((waves + NET_WAVES - 1) / NET_WAVES); }

template <int LOGN>
int launch_net_t(rtfhe_ctx* ctx, const CmuxNetArgs& a, int what, hipStream_t s) {
    const dim3 block(64 * NET_WAVES);
    constexpr size_t lds = cmux_tree_lds_bytes<LOGN, NET_WAVES>();
    if (what == 0) hipLaunchKernelGGL((k_cmux_net_check<NET_WAVES>), dim3(blocks_of((size_t)a.count)), block, 0, s, a);
    else if (what == 1 && leveled_rounded(ctx))
        hipLaunchKernelGGL((k_cmux_net<LOGN, 3, 6, NET_WAVES, true>), dim3(blocks_of((size_t)a.count * a.n_level)), block, lds, s, a);
    else if (what == 1)
        hipLaunchKernelGGL((k_cmux_net<LOGN, 3, 6, NET_WAVES, false>), dim3(blocks_of((size_t)a.count * a.n_level)), block, lds, s, a);
    else hipLaunchKernelGGL((k_cmux_net_out<LOGN, NET_WAVES>), dim3(blocks_of((size_t)a.count * a.n_out)), block, 0, s, a);
    HIPCHECK(ctx, hipGetLastError());
    ctx->launches++;
    return 0;
}

// what: 0 = k_cmux_net_check, 1 = k_cmux_net (one level; the twin of the leveled mode in force: the graph keeps it), 2 = k_cmux_net_out
int launch_net(rtfhe_ctx* ctx, const CmuxNetArgs& a, int what, hipStream_t s) {
    return ctx->logn == 11 ? launch_net_t<11>(ctx, a, what, s) : launch_net_t<10>(ctx, a, what, s);
}

}  // namespace

extern "C" {

int rtfhe_cmux_circuit_create(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const rtfhe_lut* lut, const int32_t* var, const int32_t* hi, const int32_t* lo,
                              const int32_t* rot, int32_t n_nodes, int32_t n_vars, const int32_t* out_ref, const int32_t* out_coef, int32_t n_out,
                              const void* d_sel_idx, const void* d_row0, void* d_out, size_t count, rtfhe_circuit** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!sel) return fail(ctx, RTFHE_ERR_INVALID, "null selector set (rtfhe_trgsw)");
    if (!lut) return fail(ctx, RTFHE_ERR_INVALID, "null table (rtfhe_lut)");
    if (!var || !hi || !lo || !out_ref || !d_out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (!sel->ctx || !lut->ctx) return fail(ctx, RTFHE_ERR_STATE, "the context of the selector set or of the table has been destroyed");
    if (sel->ctx != ctx) return fail(ctx, RTFHE_ERR_INVALID, "the selector set belongs to another context");
    if (lut->ctx != ctx) return fail(ctx, RTFHE_ERR_INVALID, "the table belongs to another context");
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "CMUX netlists run on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); select it with rtfhe_set_backend");
    if (n_nodes < 1 || n_vars < 1 || n_out < 1 || count < 1)
        return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_cmux_circuit_create: n_nodes, n_vars, n_out and count must be at least 1");
    // the whole description is checked and levelised before anything is allocated, captured or launched
    const rtfhe_cmux_net_world world{ctx->p.N, lut->n_lut, sel->n_sel, d_row0 ? 1 : 0, d_sel_idx ? 1 : 0, count};
    std::vector<int32_t> order((size_t)n_nodes), level_off((size_t)n_nodes + 1);
    int32_t n_levels = 0, leaf_span[2] = {0, 0};
    size_t node_bytes = 0;
    char why[320];
    if (int rc = rtfhe_cmux_net_plan(&world, var, hi, lo, rot, n_nodes, n_vars, out_ref, out_coef, n_out, order.data(), level_off.data(), &n_levels, leaf_span,
                                     &node_bytes, why, sizeof why))
        return fail(ctx, rc, why);
    const bool extract = out_coef != nullptr;
    if (extract && !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    if (int rc = use(ctx)) return rc;
    if (!gpu_accessible(ctx, d_out) || (d_sel_idx && !gpu_accessible(ctx, d_sel_idx)) || (d_row0 && !gpu_accessible(ctx, d_row0)))
        return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_cmux_circuit_create needs device pointers (got memory the GPU cannot address)");
    // everything that allocates or synchronises happens now, outside the capture
    if (int rc = ctx->logn == 11 ? prime_net_t<11>(ctx) : prime_net_t<10>(ctx)) return rc;
    rtfhe_circuit* c = new (std::nothrow) rtfhe_circuit();
    if (!c) return fail(ctx, RTFHE_ERR_NOMEM, "out of host memory");
    c->ctx = ctx; c->device = ctx->device; c->waves = n_levels; c->backend = ctx->backend; c->sel = sel;
    auto bail = [&](int rc) { circuit_release(c); delete c; return rc; };
    const size_t samples = count * (size_t)n_out, n1 = (size_t)ctx->p.n + 1;
    rtfhe_ctx::Tlwe1 cbuf;
    if (extract) {
        if (int rc = ensure_tlwe1(ctx, cbuf, samples)) return bail(rc);
        c->d_samples = cbuf.d;
    }
    // description: var, hi, lo, rot, order [n_nodes] each | out_ref, out_coef [n_out] each
    const size_t desc_words = (size_t)n_nodes * 5 + (size_t)n_out * 2;
    std::vector<int32_t> desc(desc_words, 0);
    std::memcpy(&desc[0], var, (size_t)n_nodes * 4);
    std::memcpy(&desc[(size_t)n_nodes], hi, (size_t)n_nodes * 4);
    std::memcpy(&desc[(size_t)n_nodes * 2], lo, (size_t)n_nodes * 4);
    if (rot) std::memcpy(&desc[(size_t)n_nodes * 3], rot, (size_t)n_nodes * 4);
    std::memcpy(&desc[(size_t)n_nodes * 4], order.data(), (size_t)n_nodes * 4);
    std::memcpy(&desc[(size_t)n_nodes * 5], out_ref, (size_t)n_out * 4);
    if (out_coef) std::memcpy(&desc[(size_t)n_nodes * 5 + n_out], out_coef, (size_t)n_out * 4);
    void *d_desc = nullptr, *d_nodes = nullptr, *d_ok = nullptr, *d_tv = nullptr;
    const size_t tv_bytes = (size_t)lut->n_lut * ctx->p.N * (lut->encrypted ? 2 : 1) * 4;      // an encrypted table's rows are TRLWEs: 2N words
    const std::pair<void**, size_t> bufs[] = {{&d_desc, desc_words * 4}, {&d_nodes, node_bytes}, {&d_ok, count * 4}, {&d_tv, tv_bytes}};
    for (const auto& [pp, bytes] : bufs) {
        if (hipMalloc(pp, bytes) != hipSuccess) { (void)hipGetLastError(); return bail(fail(ctx, RTFHE_ERR_HIP, "rtfhe_cmux_circuit_create: hipMalloc")); }
        c->d_owned.push_back(*pp);
    }
    if (hipMemcpy(d_desc, desc.data(), desc_words * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_tv, lut->d_tv[0], tv_bytes, hipMemcpyDeviceToDevice) != hipSuccess || hipMemset(d_ok, 0, count * 4) != hipSuccess) {
        (void)hipGetLastError();
        return bail(fail(ctx, RTFHE_ERR_HIP, "rtfhe_cmux_circuit_create: hipMemcpy / hipMemset"));
    }
    const int32_t* dd = (const int32_t*)d_desc;
    CmuxNetArgs a{};
    a.tw = ctx->d_tw; a.sel = sel->d_spec; a.sel_idx = (const int32_t*)d_sel_idx; a.row0 = (const int32_t*)d_row0; a.table = (const uint32_t*)d_tv;
    a.nodes = (uint32_t*)d_nodes; a.ok = (int32_t*)d_ok;
    a.var = dd; a.hi = dd + n_nodes; a.lo = dd + (size_t)n_nodes * 2; a.rot = rot ? dd + (size_t)n_nodes * 3 : nullptr;
    a.out_ref = dd + (size_t)n_nodes * 5; a.out_coef = extract ? dd + (size_t)n_nodes * 5 + n_out : nullptr;
    a.out = extract ? nullptr : (uint32_t*)d_out; a.ext = extract ? cbuf.d : nullptr; a.fault = ctx->d_fault;
    a.count = (int32_t)count; a.n_nodes = n_nodes; a.n_vars = n_vars; a.n_out = n_out; a.n_sel = sel->n_sel; a.n_lut = lut->n_lut;
    a.leaf_min = leaf_span[0]; a.leaf_max = leaf_span[1]; a.enc = lut->encrypted ? 1 : 0;
    const int64_t before = ctx->launches;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return bail(fail(ctx, RTFHE_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e)));
    e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return bail(fail(ctx, RTFHE_ERR_HIP, std::string("hipStreamBeginCapture: ") + hipGetErrorString(e)));
    ctx->tlwe1_capture = &cbuf;      // (the key switch brackets nothing with timer events inside a circuit's capture)
    int rc = launch_net(ctx, a, 0, ctx->stream);
    for (int32_t k = 0; k < n_levels && !rc; k++) {
        a.level = dd + (size_t)n_nodes * 4 + level_off[(size_t)k];
        a.n_level = level_off[(size_t)k + 1] - level_off[(size_t)k];
        rc = launch_net(ctx, a, 1, ctx->stream);
    }
    if (!rc) rc = launch_net(ctx, a, 2, ctx->stream);
    if (!rc && extract) {
        // identity_key_switch of the count * n_out samples, as the tree's extract form does it
        if (!ctx->d_ksmat) {
            rc = launch_key_switch_ext(ctx, cbuf.d, (uint32_t*)d_out, samples, ctx->stream);
        } else {
            if (hipMemsetAsync(d_out, 0, samples * n1 * 4, ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_cmux_circuit_create: hipMemsetAsync");
            BootstrapArgs k{};
            k.out = (uint32_t*)d_out; k.count = (int32_t)samples; k.n = ctx->p.n;
            if (!rc) rc = launch_key_switch_mm(ctx, k, cbuf.d, ctx->stream);
        }
    }
    ctx->tlwe1_capture = nullptr;
    e = hipStreamEndCapture(ctx->stream, &c->graph);
    c->launches = ctx->launches - before;
    ctx->launches = before;
    if (rc) return bail(rc);
    if (e != hipSuccess) return bail(fail(ctx, RTFHE_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e)));
    e = hipGraphInstantiate(&c->exec, c->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) return bail(fail(ctx, RTFHE_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e)));
    ctx->circuits.push_back(c);
    *out = c;
    return 0;
}

// rtfhe_trgsw_create's conversion of selectors [first, first + n) of a live set, in place and synchronous
int rtfhe_trgsw_update(rtfhe_trgsw* sel, const uint32_t* trgsw, int32_t first, int32_t n) {
    if (!sel) return fail(nullptr, RTFHE_ERR_INVALID, "null selector set (rtfhe_trgsw)");
    rtfhe_ctx* ctx = sel->ctx;
    if (!ctx) return fail(nullptr, RTFHE_ERR_STATE, "the context of the selector set has been destroyed");
    if (!trgsw) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (first < 0 || n < 1 || (long long)first + n > sel->n_sel)
        return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trgsw_update: selectors [" + std::to_string(first) + ", " + std::to_string((long long)first + n) +
                                            ") are outside the set's [0, " + std::to_string(sel->n_sel) + ")");
    if (int rc = use(ctx)) return rc;
    const size_t polys = (size_t)n * 2 * 2 * ctx->p.l, words = polys * ctx->p.N, per_sel = (size_t)2 * 2 * ctx->p.l * (ctx->p.N / 2);
    HIPCHECK(ctx, hipDeviceSynchronize());            // replays on any stream may still read the old spectra
    if (int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, words * 4)) return rc;
    HIPCHECK(ctx, hipMemcpy(ctx->d_a, trgsw, words * 4, hipMemcpyHostToDevice));
    if (int rc = launch_fft(ctx, true, FftArgs{ctx->d_tw, ctx->d_a, sel->d_spec + (size_t)first * per_sel, (int32_t)polys, 1, 2 * ctx->p.l, 0}, ctx->stream)) return rc;
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
