// rtfhe_cmux_tree.hip -- CMUX-tree table lookup with caller-supplied TRGSW selectors (include/rtfhe.h: rtfhe_trgsw_create,
// rtfhe_cmux_tree_batch[_dev], rtfhe_cmux_tree_extract_batch[_dev]): selector sets, the argument checks, the stream's ping-pong buffers
// and the rules around stream captures, one launch of k_cmux_tree per level (its ROUNDED twin in the rounded leveled mode,
// rtfhe_set_leveled_decomposition), and for the extract form the batch key switch many-LUT uses.
// Beside it the TRGSW blind rotation (rtfhe_trgsw_rotate_batch[_dev], rtfhe_trgsw_rotate_extract_batch[_dev]): the same selector sets, one
// launch of k_trgsw_rotate for all steps of all lookups, the same key switch behind the extract form.
// And the tree run backwards, the CMUX demultiplexer (rtfhe_demux_tree_batch[_dev]): one launch of k_demux_tree per level through the same
// ping-pong buffers.  (Its leaves go into an encrypted table's rows through rtfhe_lut_accumulate_dev, rtfhe_lut.hip.)
#include "rtfhe_host.hpp"

#include <cstdlib>

#include "rtfhe_kernels_cmux_tree.hpp"
#include "rtfhe_kernels_demux_tree.hpp"
#include "rtfhe_kernels_trgsw_rotate.hpp"
#include "rtfhe_plan_kit.hpp"

using namespace rtfhe;
using namespace rtfhe_host;
using rtfhe_plan::rows_overlap;

namespace {

// the three families' twins, four waves (= nodes) per workgroup at both N, on k_cmux_tree's LDS carve
RTFHE_LEVELED_FAMILY(tree_twins, CmuxTreeArgs, k_cmux_tree, cmux_tree_lds_bytes<LOGN, LEVELED_WAVES>())
RTFHE_LEVELED_FAMILY(demux_twins, DemuxTreeArgs, k_demux_tree, cmux_tree_lds_bytes<LOGN, LEVELED_WAVES>())
RTFHE_LEVELED_FAMILY(rotate_twins, TrgswRotateArgs, k_trgsw_rotate, cmux_tree_lds_bytes<LOGN, LEVELED_WAVES>())

// ---- the argument checks every entry over a selector set shares, after selector_set_ready and in this order ----
// depth, and count against the 2^31 nodes (doubling: a tree's levels) or steps (a rotation's) one launch can number
int depth_ready(rtfhe_ctx* ctx, int32_t depth, size_t count, bool doubling) {
    if (depth < 1 || depth > CMUX_TREE_MAX_DEPTH) return fail(ctx, RTFHE_ERR_INVALID, "depth = " + std::to_string(depth) + " is outside [1, 16]");
    if (doubling && count > ((size_t)0x7fffffff >> (depth - 1))) return fail(ctx, RTFHE_ERR_INVALID, "count * 2^(depth-1) too large");
    if (!doubling && count > (size_t)0x7fffffff / (size_t)depth) return fail(ctx, RTFHE_ERR_INVALID, "count * depth too large");
    return 0;
}
// the selector indices: host_sel_idx is the host-side array (null in the _dev forms, whose array the kernel checks)
int sel_idx_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, int32_t depth, size_t count, bool has_sel_idx, const int32_t* host_sel_idx) {
    const long long n_sel = sel->n_sel;
    if (!has_sel_idx && (long long)count * depth > n_sel)
        return fail(ctx, RTFHE_ERR_INVALID, "sel_idx NULL: lookup " + std::to_string(count - 1) + " needs selectors up to " + std::to_string((long long)count * depth - 1) +
                                            ", the set has " + std::to_string(n_sel));
    if (host_sel_idx)
        for (size_t g = 0; g < count; g++)
            for (int k = 0; k < depth; k++)
                if ((uint32_t)host_sel_idx[g * depth + k] >= (uint32_t)sel->n_sel)
                    return fail(ctx, RTFHE_ERR_INVALID, "lookup " + std::to_string(g) + ": sel_idx[" + std::to_string(k) + "] = " + std::to_string(host_sel_idx[g * depth + k]) +
                                                        " is outside [0, " + std::to_string(n_sel) + ")");
    return 0;
}

// the ping-pong buffers of a tree's or a demultiplexer's levels on stream s, `need` words each (0: a single level, no buffer, nothing to refuse)
int level_buffers(rtfhe_ctx* ctx, hipStream_t s, bool in_capture, size_t need, const char* refusal, StreamScratch*& out) {
    out = nullptr;
    return need ? stream_scratch(ctx, ctx->tree, s, in_capture, ScratchShape{2, 4}, need, refusal, out) : 0;
}

// ---- CMUX tree ----
// what every tree entry checks before anything is allocated or launched; host_* are the host-side index arrays (null in the _dev forms, whose
// arrays are checked by the kernel), out the caller's result buffer
int tree_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const rtfhe_lut* lut, int32_t depth, size_t count, bool has_sel_idx, bool has_row0,
               const int32_t* host_sel_idx, const int32_t* host_row0, const int32_t* host_coef, const void* out, bool extract) {
    if (int rc = selector_set_ready(ctx, sel, true, lut, out != nullptr, "the CMUX tree runs")) return rc;
    if (int rc = depth_ready(ctx, depth, count, true)) return rc;
    if (extract && !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    const long long rows = 1ll << depth, n_lut = lut->n_lut;
    if (!has_row0 && rows > n_lut)
        return fail(ctx, RTFHE_ERR_INVALID, "a depth-" + std::to_string(depth) + " tree reads " + std::to_string(rows) + " rows, the table has " + std::to_string(n_lut));
    if (int rc = sel_idx_ready(ctx, sel, depth, count, has_sel_idx, host_sel_idx)) return rc;
    for (size_t g = 0; g < count; g++) {
        if (host_row0 && (host_row0[g] < 0 || (long long)host_row0[g] + rows > n_lut))
            return fail(ctx, RTFHE_ERR_INVALID, "lookup " + std::to_string(g) + ": row0 = " + std::to_string(host_row0[g]) + " with " + std::to_string(rows) +
                                                " rows is outside the table's [0, " + std::to_string(n_lut) + ")");
        if (host_coef && (uint32_t)host_coef[g] >= (uint32_t)ctx->p.N)
            return fail(ctx, RTFHE_ERR_INVALID, "lookup " + std::to_string(g) + ": coef = " + std::to_string(host_coef[g]) + " is outside [0, " + std::to_string(ctx->p.N) + ")");
    }
    return 0;
}

// The tree of `count` lookups on device buffers, primary device, stream s.  d_out: [count][2][N], or in the extract form [count][n+1].
int launch_tree(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* d_sel_idx, int32_t depth, const rtfhe_lut* lut, const int32_t* d_row0,
                const int32_t* d_coef, void* d_out, size_t count, bool extract, hipStream_t s) {
    if (count == 0) return 0;
    const size_t N = (size_t)ctx->p.N, need = depth > 1 ? (count << (depth - 1)) * 2 * N : 0;      // words of each ping-pong buffer
    const bool cap = capturing(s);
    StreamScratch *pp = nullptr, *samples = nullptr;
    if (int rc = level_buffers(ctx, s, cap, need, "a CMUX tree inside a stream capture needs this stream's ping-pong buffers to exist already: run one eager "
                                                  "rtfhe_cmux_tree_batch_dev of at least this count and depth on the stream before capturing", pp))
        return rc;
    if (extract)
        if (int rc = stream_scratch(ctx, ctx->tlwe1, s, cap, tlwe1_shape(ctx), count,
                                    "a CMUX tree with extraction inside a stream capture needs this stream's sample buffer to exist already: run one "
                                    "eager rtfhe_cmux_tree_extract_batch_dev of at least this count on the stream before capturing", samples, ctx->tlwe1_capture))
            return rc;
    CmuxTreeArgs a{};
    a.tw = ctx->d_tw; a.sel = sel->d_spec; a.sel_idx = d_sel_idx; a.row0 = d_row0; a.coef = extract ? d_coef : nullptr;
    a.table = lut->d_tv[0]; a.fault = ctx->d_fault;
    a.count = (int32_t)count; a.depth = depth; a.n_sel = sel->n_sel; a.n_lut = lut->n_lut; a.enc = lut->encrypted ? 1 : 0;
    const LeveledTwins<CmuxTreeArgs> k = tree_twins(ctx);
    for (int level = 0; level < depth; level++) {
        const bool last = level == depth - 1;
        a.level = level;
        a.src = level ? pp->d[(level - 1) & 1] : nullptr;
        a.dst = last ? (extract ? nullptr : (uint32_t*)d_out) : pp->d[level & 1];
        a.ext = last && extract ? samples->d[0] : nullptr;
        if (int rc = launch_leveled(ctx, k, count << (depth - 1 - level), s, a)) return rc;
    }
    // identity_key_switch of the count samples, as a many-LUT PBS does it (launch_pbs_many, rtfhe_batch.hip)
    return extract ? launch_key_switch_rows(ctx, samples->d[0], (uint32_t*)d_out, count, s) : 0;
}

int tree_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const rtfhe_lut* lut, const void* d_row0, const void* d_coef,
             void* d_out, size_t count, bool extract, void* stream, const char* name) {
    if (int rc = tree_ready(ctx, sel, lut, depth, count, d_sel_idx != nullptr, d_row0 != nullptr, nullptr, nullptr, nullptr, d_out, extract)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, name, {d_out}, {d_sel_idx, d_row0, d_coef})) return rc;
    return launch_tree(ctx, sel, (const int32_t*)d_sel_idx, depth, lut, (const int32_t*)d_row0, (const int32_t*)d_coef, d_out, count, extract, (hipStream_t)stream);
}

// host buffers: the index arrays ride in the staging buffers (sel_idx in d_a; row0 then coef in d_b), the result comes back through d_c
int tree_host(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const rtfhe_lut* lut, const int32_t* row0, const int32_t* coef,
              uint32_t* out, size_t count, bool extract) {
    if (int rc = tree_ready(ctx, sel, lut, depth, count, sel_idx != nullptr, row0 != nullptr, sel_idx, row0, coef, out, extract)) return rc;
    const size_t out_bytes = count * (extract ? (size_t)ctx->p.n + 1 : (size_t)2 * ctx->p.N) * 4;
    return host_form(ctx, count, {staging_a(ctx), nullptr, 0}, {staging_c(ctx), out, out_bytes, false},
                     {{staging_a(ctx), count * depth, sel_idx, nullptr}, {staging_b(ctx), count, row0, coef}}, [&](const void*, const StagedIdx* idx, void* d_out) {
        return launch_tree(ctx, sel, idx[0].first, depth, lut, idx[1].first, idx[1].second, d_out, count, extract, ctx->stream);
    });
}

// ---- CMUX demultiplexer tree ----
// what both demultiplexer entries check before anything is allocated or launched; host_sel_idx is null in the _dev form, whose array the kernel checks
int demux_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, int32_t depth, size_t count, bool has_sel_idx, const int32_t* host_sel_idx, const void* x, const void* out) {
    if (int rc = selector_set_ready(ctx, sel, false, nullptr, x && out, "the CMUX demultiplexer runs")) return rc;
    if (int rc = depth_ready(ctx, depth, count, true)) return rc;
    return sel_idx_ready(ctx, sel, depth, count, has_sel_idx, host_sel_idx);
}

// The demultiplexer of `count` TRLWEs on device buffers, primary device, stream s.  d_x: [count][2][N], d_out: [count][2^depth][2][N].  Level t
// reads count << t nodes and writes twice as many; levels 0 .. depth-2 alternate between the stream's ping-pong buffers (the tree's, under the
// tree's rules), the last level writes d_out.
int launch_demux(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* d_sel_idx, int32_t depth, const void* d_x, void* d_out, size_t count, hipStream_t s) {
    if (count == 0) return 0;
    const size_t N = (size_t)ctx->p.N, need = depth > 1 ? (count << (depth - 1)) * 2 * N : 0;      // words of each ping-pong buffer
    StreamScratch* pp = nullptr;
    if (int rc = level_buffers(ctx, s, capturing(s), need, "a CMUX demultiplexer inside a stream capture needs this stream's ping-pong buffers to exist already: run one eager "
                                                           "rtfhe_demux_tree_batch_dev of at least this count and depth on the stream before capturing", pp))
        return rc;
    DemuxTreeArgs a{};
    a.tw = ctx->d_tw; a.sel = sel->d_spec; a.sel_idx = d_sel_idx; a.fault = ctx->d_fault;
    a.count = (int32_t)count; a.depth = depth; a.n_sel = sel->n_sel;
    const LeveledTwins<DemuxTreeArgs> k = demux_twins(ctx);
    for (int level = 0; level < depth; level++) {
        a.level = level;
        a.src = level ? pp->d[(level - 1) & 1] : (const uint32_t*)d_x;
        a.dst = level == depth - 1 ? (uint32_t*)d_out : pp->d[level & 1];
        if (int rc = launch_leveled(ctx, k, count << level, s, a)) return rc;
    }
    return 0;
}

// ---- TRGSW blind rotation ----
// what every rotation entry checks before anything is allocated or launched; host_sel_idx is null in the _dev forms, whose array the kernel checks
int rotate_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, int32_t depth, const int32_t* rot, size_t count, bool has_sel_idx, const int32_t* host_sel_idx,
                 const void* in, const void* out, bool extract) {
    if (int rc = selector_set_ready(ctx, sel, false, nullptr, in && out, "the TRGSW rotation runs")) return rc;
    if (int rc = depth_ready(ctx, depth, count, false)) return rc;
    const int N = ctx->p.N;
    if (rot) {
        for (int k = 0; k < depth; k++)
            if (rot[k] < 0 || rot[k] >= 2 * N)
                return fail(ctx, RTFHE_ERR_INVALID, "step " + std::to_string(k) + ": rot = " + std::to_string(rot[k]) + " is outside [0, " + std::to_string(2 * N) + ")");
    } else if (depth > ctx->logn + 1) {
        return fail(ctx, RTFHE_ERR_INVALID, "rot NULL: step " + std::to_string(ctx->logn + 1) + " would rotate by X^-2^" + std::to_string(ctx->logn + 1) +
                                            " = 1; depth = " + std::to_string(depth) + " is above log2 N + 1 = " + std::to_string(ctx->logn + 1));
    }
    if (extract && !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    return sel_idx_ready(ctx, sel, depth, count, has_sel_idx, host_sel_idx);
}

// The rotation of `count` TRLWEs on device buffers, primary device, stream s.  d_out: [count][2][N] (may be d_in), or in the extract form [count][n+1].
// The plain form allocates nothing; the extract form needs the stream's lvl1 sample buffer, under the tree's rule inside a capture.
int launch_rotate(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* d_sel_idx, int32_t depth, const int32_t* rot, const void* d_in, void* d_out, size_t count,
                  bool extract, hipStream_t s) {
    if (count == 0) return 0;
    StreamScratch* samples = nullptr;
    if (extract)
        if (int rc = stream_scratch(ctx, ctx->tlwe1, s, capturing(s), tlwe1_shape(ctx), count,
                                    "a TRGSW rotation with extraction inside a stream capture needs this stream's sample buffer to exist already: run one "
                                    "eager rtfhe_trgsw_rotate_extract_batch_dev of at least this count on the stream before capturing", samples, ctx->tlwe1_capture))
            return rc;
    TrgswRotateArgs a{};
    a.tw = ctx->d_tw; a.sel = sel->d_spec; a.sel_idx = d_sel_idx; a.in = (const uint32_t*)d_in; a.fault = ctx->d_fault;
    a.out = extract ? nullptr : (uint32_t*)d_out;
    a.ext = extract ? samples->d[0] : nullptr;
    a.ks_out = extract ? (uint32_t*)d_out : nullptr;
    a.count = (int32_t)count; a.depth = depth; a.n_sel = sel->n_sel; a.n = ctx->p.n;
    for (int k = 0; k < depth; k++) a.rot[k] = rot ? rot[k] : 2 * ctx->p.N - (1 << k);      // NULL: X^{-2^k}
    if (int rc = launch_leveled(ctx, rotate_twins(ctx), count, s, a)) return rc;
    if (!extract) return 0;
    // identity_key_switch of the count samples, as the tree's extract form does it; then the rows of skipped lookups as they were (counted, and
    // launched with a null sel_idx too: a rotation with extraction is three launches)
    return launch_key_switch_rows_restore(ctx, samples->d[0], (uint32_t*)d_out, count, d_sel_idx, depth, sel->n_sel, true, s);
}

int rotate_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const int32_t* rot, const void* d_trlwe, void* d_out, size_t count,
               bool extract, void* stream, const char* name) {
    if (int rc = rotate_ready(ctx, sel, depth, rot, count, d_sel_idx != nullptr, nullptr, d_trlwe, d_out, extract)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, name, {d_out, d_trlwe}, {d_sel_idx})) return rc;
    const size_t in_bytes = count * 2 * (size_t)ctx->p.N * 4, out_bytes = extract ? count * ((size_t)ctx->p.n + 1) * 4 : in_bytes;
    if (d_out != d_trlwe ? rows_overlap(d_trlwe, in_bytes, d_out, out_bytes) : extract)
        return fail(ctx, RTFHE_ERR_INVALID, std::string(name) + ": d_out overlaps d_trlwe (it may only be exactly d_trlwe, in the form without extraction)");
    return launch_rotate(ctx, sel, (const int32_t*)d_sel_idx, depth, rot, d_trlwe, d_out, count, extract, (hipStream_t)stream);
}

// host buffers: sel_idx rides in d_a, the rows in d_b, the result comes back through d_c
int rotate_host(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const int32_t* rot, const uint32_t* trlwe, uint32_t* out, size_t count,
                bool extract) {
    if (int rc = rotate_ready(ctx, sel, depth, rot, count, sel_idx != nullptr, sel_idx, trlwe, out, extract)) return rc;
    const size_t in_bytes = count * 2 * (size_t)ctx->p.N * 4, out_bytes = extract ? count * ((size_t)ctx->p.n + 1) * 4 : in_bytes;
    return host_form(ctx, count, {staging_b(ctx), trlwe, in_bytes}, {staging_c(ctx), out, out_bytes, false}, {{staging_a(ctx), count * depth, sel_idx, nullptr}},
                     [&](const void* d_trlwe, const StagedIdx* idx, void* d_out) {
        return launch_rotate(ctx, sel, idx[0].first, depth, rot, d_trlwe, d_out, count, extract, ctx->stream);
    });
}

}  // namespace

namespace rtfhe_host {

int selector_set_ready(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, bool with_table, const rtfhe_lut* lut, bool args_ok, const char* who) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = with_table ? handles_ready(ctx, {ref(sel), ref(lut)}) : handles_ready(ctx, {ref(sel)})) return rc;
    if (!args_ok) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, std::string(who) + " on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); select it with rtfhe_set_backend");
    return 0;
}

void trgsw_release(rtfhe_trgsw* t) {
    (void)hipSetDevice(t->ctx->device);
    if (t->d_spec) (void)hipFree(t->d_spec);
    t->d_spec = nullptr;
}

// TRGSWRepF::from (trgsw.rs:68-76) of n samples, as rtfhe_load_bk_torus converts the bootstrapping key: the forward transform of the words
// viewed as signed i32, written in the canonical device layout [2l][2][R][64] at dst_spec.  Queued on ctx->stream: ctx->d_a grown to the
// samples' words, stage(words) -- what brings them there: the caller's copy, or a seeded form's expansion --, the transform.  The caller waits
// for the stream (rtfhe_trgsw_create and rtfhe_trgsw_update word that failure differently).
int convert_selectors(rtfhe_ctx* ctx, cplx* dst_spec, int32_t n, const std::function<int(size_t)>& stage) {
    const size_t polys = (size_t)n * 2 * 2 * ctx->p.l, words = polys * ctx->p.N;
    if (int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, words * 4)) return rc;
    if (int rc = stage(words)) return rc;
    return launch_fft(ctx, true, FftArgs{ctx->d_tw, ctx->d_a, dst_spec, (int32_t)polys, 1, 2 * ctx->p.l, 0}, ctx->stream);
}

}  // namespace rtfhe_host

// a new selector set: what only creation does around convert_selectors
static int trgsw_create_staged(rtfhe_ctx* ctx, int32_t n_sel, rtfhe_trgsw** out, const std::function<int(size_t)>& stage) {
    *out = nullptr;
    if (int rc = use(ctx)) return rc;
    // the rotation, the demultiplexer and the TRLWE x TRGSW product are granted their dynamic LDS now, so that the first of a context may already
    // sit in a stream capture
    if (int rc = prime_leveled(ctx, rotate_twins(ctx))) return rc;
    if (int rc = prime_leveled(ctx, demux_twins(ctx))) return rc;
    if (int rc = prime_trgsw_mac(ctx)) return rc;
    const size_t polys = (size_t)n_sel * 2 * 2 * ctx->p.l, words = polys * ctx->p.N;
    if (polys > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trgsw_create: n_sel too large");
    NewHandle<rtfhe_trgsw> t = new_handle(ctx, trgsw_release);
    t->n_sel = n_sel;
    int rc = hipMalloc((void**)&t->d_spec, words / 2 * sizeof(cplx)) == hipSuccess ? 0 : fail(ctx, RTFHE_ERR_HIP, "rtfhe_trgsw_create: hipMalloc");
    if (!rc) rc = convert_selectors(ctx, t->d_spec, n_sel, stage);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_trgsw_create: hipStreamSynchronize");
    return rc ? rc : handle_publish(ctx->trgsws, std::move(t), out);
}

extern "C" {

int rtfhe_trgsw_create(rtfhe_ctx* ctx, const uint32_t* trgsw, int32_t n_sel, rtfhe_trgsw** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!trgsw || !out || n_sel < 1) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trgsw_create: null argument or n_sel < 1");
    return trgsw_create_staged(ctx, n_sel, out, [&](size_t words) { return copy_in(ctx, ctx->d_a, trgsw, words * 4, 0); });
}

// the same set from its seeded form: the b halves go up, the masks are made on the device
int rtfhe_trgsw_create_seeded(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* b, int32_t n_sel, rtfhe_trgsw** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!seed || !b || !out || n_sel < 1) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trgsw_create_seeded: null argument or n_sel < 1");
    const int group = 2 * ctx->p.l;
    const size_t rows = (size_t)n_sel * group;
    if (int rc = seeded_ready(ctx, "rtfhe_trgsw_create_seeded", RTFHE_SEEDED_UPLOAD, seed, first_row, b, group, nullptr, rows)) return rc;
    return trgsw_create_staged(ctx, n_sel, out, [&](size_t) { return stage_seeded(ctx, seed, first_row, b, group, rows, ctx->d_a); });
}

void rtfhe_trgsw_destroy(rtfhe_trgsw* t) {
    handle_destroy(&rtfhe_ctx::trgsws, t, trgsw_release, [t](rtfhe_ctx* ctx) {
        for (rtfhe_circuit* c : ctx->circuits) if (c->sel == t) { c->sel = nullptr; c->sel_gone = true; }      // CMUX netlists recorded on this set
    });
}

int rtfhe_cmux_tree_batch(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const rtfhe_lut* lut, const int32_t* row0,
                          uint32_t* out, size_t count) {
    return tree_host(ctx, sel, sel_idx, depth, lut, row0, nullptr, out, count, false);
}

int rtfhe_cmux_tree_batch_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const rtfhe_lut* lut, const void* d_row0,
                              void* d_out, size_t count, void* stream) {
    return tree_dev(ctx, sel, d_sel_idx, depth, lut, d_row0, nullptr, d_out, count, false, stream, "rtfhe_cmux_tree_batch_dev");
}

int rtfhe_cmux_tree_extract_batch(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const rtfhe_lut* lut, const int32_t* row0,
                                  const int32_t* coef, uint32_t* out, size_t count) {
    return tree_host(ctx, sel, sel_idx, depth, lut, row0, coef, out, count, true);
}

int rtfhe_cmux_tree_extract_batch_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const rtfhe_lut* lut, const void* d_row0,
                                      const void* d_coef, void* d_out, size_t count, void* stream) {
    return tree_dev(ctx, sel, d_sel_idx, depth, lut, d_row0, d_coef, d_out, count, true, stream, "rtfhe_cmux_tree_extract_batch_dev");
}

int rtfhe_demux_tree_batch(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const uint32_t* x, uint32_t* out, size_t count) {
    if (int rc = demux_ready(ctx, sel, depth, count, sel_idx != nullptr, sel_idx, x, out)) return rc;
    // host buffers: sel_idx rides in d_a, the inputs in d_b, the leaves come back through d_c
    const size_t in_bytes = count * 2 * (size_t)ctx->p.N * 4, out_bytes = in_bytes << depth;
    return host_form(ctx, count, {staging_b(ctx), x, in_bytes}, {staging_c(ctx), out, out_bytes, false}, {{staging_a(ctx), count * depth, sel_idx, nullptr}},
                     [&](const void* d_x, const StagedIdx* idx, void* d_out) { return launch_demux(ctx, sel, idx[0].first, depth, d_x, d_out, count, ctx->stream); });
}

int rtfhe_demux_tree_batch_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const void* d_x, void* d_out, size_t count,
                               void* stream) {
    if (int rc = demux_ready(ctx, sel, depth, count, d_sel_idx != nullptr, nullptr, d_x, d_out)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, "rtfhe_demux_tree_batch_dev", {d_out, d_x}, {d_sel_idx})) return rc;
    const size_t in_bytes = count * 2 * (size_t)ctx->p.N * 4, out_bytes = in_bytes << depth;
    if (rows_overlap(d_x, in_bytes, d_out, out_bytes))      // the last level stores leaves while other waves still read their nodes (depth 1: x itself)
        return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_demux_tree_batch_dev: d_out overlaps d_x");
    return launch_demux(ctx, sel, (const int32_t*)d_sel_idx, depth, d_x, d_out, count, (hipStream_t)stream);
}

int rtfhe_trgsw_rotate_batch(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const int32_t* rot, const uint32_t* trlwe,
                             uint32_t* out, size_t count) {
    return rotate_host(ctx, sel, sel_idx, depth, rot, trlwe, out, count, false);
}

int rtfhe_trgsw_rotate_batch_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const int32_t* rot, const void* d_trlwe,
                                 void* d_out, size_t count, void* stream) {
    return rotate_dev(ctx, sel, d_sel_idx, depth, rot, d_trlwe, d_out, count, false, stream, "rtfhe_trgsw_rotate_batch_dev");
}

int rtfhe_trgsw_rotate_extract_batch(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const int32_t* sel_idx, int32_t depth, const int32_t* rot, const uint32_t* trlwe,
                                     uint32_t* out, size_t count) {
    return rotate_host(ctx, sel, sel_idx, depth, rot, trlwe, out, count, true);
}

int rtfhe_trgsw_rotate_extract_batch_dev(rtfhe_ctx* ctx, const rtfhe_trgsw* sel, const void* d_sel_idx, int32_t depth, const int32_t* rot, const void* d_trlwe,
                                         void* d_out, size_t count, void* stream) {
    return rotate_dev(ctx, sel, d_sel_idx, depth, rot, d_trlwe, d_out, count, true, stream, "rtfhe_trgsw_rotate_extract_batch_dev");
}

}  // extern "C"
