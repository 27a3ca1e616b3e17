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

RTFHE_LEVELED_FAMILY(net_twins, CmuxNetArgs, k_cmux_net, cmux_tree_lds_bytes<LOGN, LEVELED_WAVES>())      // the tree's shape and LDS carve

// k_cmux_net_check and k_cmux_net_out: no twin, no dynamic LDS, a wave per replica / per (replica, output) on the same workgroups of four waves
template <typename K>
int launch_net_plain(rtfhe_ctx* ctx, K k, size_t waves, const CmuxNetArgs& a, hipStream_t s) {
    return launch_kernel(ctx, k, dim3((unsigned)((waves + LEVELED_WAVES - 1) / LEVELED_WAVES)), dim3(64 * LEVELED_WAVES), 0, s, a);
}

}  // namespace

extern "C" {

int rtfhe_cmux_circuit_create(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const rtfhe_lut* lut, const int32_t* var, const int32_t* hi, const int32_t* lo,
                              const int32_t* rot, int32_t n_nodes, int32_t n_vars, const int32_t* out_ref, const int32_t* out_coef, int32_t n_out,
                              const void* d_sel_idx, const void* d_row0, void* d_out, size_t count, rtfhe_circuit** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = selector_set_ready(ctx, sel, true, lut, var && hi && lo && out_ref && d_out, "CMUX netlists run")) return rc;
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
    if (int rc = device_pointers(ctx, "rtfhe_cmux_circuit_create", {d_out}, {d_sel_idx, d_row0})) return rc;
    // everything that allocates or synchronises happens now, outside the capture
    const LeveledTwins<CmuxNetArgs> net = net_twins(ctx);
    if (int rc = prime_leveled(ctx, net)) return rc;
    NewCircuit c(new (std::nothrow) rtfhe_circuit());
    if (!c) return fail(ctx, RTFHE_ERR_NOMEM, "out of host memory");
    c->ctx = ctx; c->device = ctx->device; c->waves = n_levels; c->backend = ctx->backend; c->sel = sel;
    const size_t samples = count * (size_t)n_out;
    StreamScratch cbuf;
    if (extract) {
        if (int rc = ensure_tlwe1(ctx, cbuf, samples)) return rc;
        c->d_samples = cbuf.d[0];
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
    if (int rc = circuit_own(ctx, c.get(), "rtfhe_cmux_circuit_create",
                             {{&d_desc, desc_words * 4}, {&d_nodes, node_bytes}, {&d_ok, count * 4}, {&d_tv, lut_bytes(ctx, lut)}})) return rc;
    if (int rc = circuit_fill(ctx, "rtfhe_cmux_circuit_create", d_desc, desc, d_tv, lut, d_ok, count * 4)) return rc;
    const int32_t* dd = (const int32_t*)d_desc;
    CmuxNetArgs a{};
    a.tw = ctx->d_tw; a.sel = sel->d_spec; a.sel_idx = (const int32_t*)d_sel_idx; a.row0 = (const int32_t*)d_row0; a.table = (const uint32_t*)d_tv;
    a.nodes = (uint32_t*)d_nodes; a.ok = (int32_t*)d_ok;
    a.var = dd; a.hi = dd + n_nodes; a.lo = dd + (size_t)n_nodes * 2; a.rot = rot ? dd + (size_t)n_nodes * 3 : nullptr;
    a.out_ref = dd + (size_t)n_nodes * 5; a.out_coef = extract ? dd + (size_t)n_nodes * 5 + n_out : nullptr;
    a.out = extract ? nullptr : (uint32_t*)d_out; a.ext = extract ? cbuf.d[0] : nullptr; a.fault = ctx->d_fault;
    a.count = (int32_t)count; a.n_nodes = n_nodes; a.n_vars = n_vars; a.n_out = n_out; a.n_sel = sel->n_sel; a.n_lut = lut->n_lut;
    a.leaf_min = leaf_span[0]; a.leaf_max = leaf_span[1]; a.enc = lut->encrypted ? 1 : 0;
    // recorded by circuit_record, under its rule; &cbuf also in the TRLWE form: the key switch brackets nothing with timer events inside a circuit's capture
    return circuit_record(ctx, std::move(c), &cbuf, out, [&] {
        int rc = launch_net_plain(ctx, k_cmux_net_check<LEVELED_WAVES>, count, a, ctx->stream);
        for (int32_t k = 0; k < n_levels && !rc; k++) {
            a.level = dd + (size_t)n_nodes * 4 + level_off[(size_t)k];
            a.n_level = level_off[(size_t)k + 1] - level_off[(size_t)k];
            rc = launch_leveled(ctx, net, count * (size_t)a.n_level, ctx->stream, a);      // the twin of the leveled mode in force: the graph keeps it
        }
        if (!rc) rc = ctx->logn == 11 ? launch_net_plain(ctx, k_cmux_net_out<11, LEVELED_WAVES>, samples, a, ctx->stream)
                                      : launch_net_plain(ctx, k_cmux_net_out<10, LEVELED_WAVES>, samples, a, ctx->stream);
        // identity_key_switch of the count * n_out samples, as the tree's extract form does it
        if (!rc && extract) rc = launch_key_switch_rows(ctx, cbuf.d[0], (uint32_t*)d_out, samples, ctx->stream);
        return rc;
    });
}

}  // extern "C"

// rtfhe_trgsw_create's conversion (convert_selectors) of selectors [first, first + n) of a live set, in place and synchronous
// (args_ok: the caller's other pointers; stage: convert_selectors')
static int trgsw_update_staged(rtfhe_trgsw* sel, bool args_ok, int32_t first, int32_t n, const std::function<int(size_t)>& stage) {
    rtfhe_ctx* ctx = sel ? sel->ctx : nullptr;
    if (int rc = handles_ready(ctx, {ref(sel)})) return rc;
    if (!args_ok) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (first < 0 || n < 1 || (long long)first + n > sel->n_sel)
        return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trgsw_update: selectors [" + std::to_string(first) + ", " + std::to_string((long long)first + n) +
                                            ") are outside the set's [0, " + std::to_string(sel->n_sel) + ")");
    if (int rc = use(ctx)) return rc;
    const size_t per_sel = (size_t)2 * 2 * ctx->p.l * (ctx->p.N / 2);
    HIPCHECK(ctx, hipDeviceSynchronize());            // replays on any stream may still read the old spectra
    if (int rc = convert_selectors(ctx, sel->d_spec + (size_t)first * per_sel, n, stage)) return rc;
    HIPCHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

extern "C" {

int rtfhe_trgsw_update(rtfhe_trgsw* sel, const uint32_t* trgsw, int32_t first, int32_t n) {
    rtfhe_ctx* ctx = sel ? sel->ctx : nullptr;      // (staging runs behind the handle check)
    return trgsw_update_staged(sel, trgsw != nullptr, first, n, [&](size_t words) {
        HIPCHECK(ctx, hipMemcpy(ctx->d_a, trgsw, words * 4, hipMemcpyHostToDevice));
        return 0;
    });
}

// ... from the seeded form of the new samples (rows first_row .. of the seed, their b halves)
int rtfhe_trgsw_update_seeded(rtfhe_trgsw* sel, const uint32_t* seed, uint64_t first_row, const uint32_t* b, int32_t first, int32_t n) {
    rtfhe_ctx* ctx = sel ? sel->ctx : nullptr;
    if (ctx && seed && b && n >= 1)
        if (int rc = seeded_ready(ctx, "rtfhe_trgsw_update_seeded", RTFHE_SEEDED_UPLOAD, seed, first_row, b, 2 * ctx->p.l, nullptr, (size_t)n * 2 * ctx->p.l)) return rc;
    return trgsw_update_staged(sel, seed && b, first, n, [&](size_t) {
        return stage_seeded(ctx, seed, first_row, b, 2 * ctx->p.l, (size_t)n * 2 * ctx->p.l, ctx->d_a);
    });
}

}  // extern "C"
