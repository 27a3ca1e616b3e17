// rtfhe_batch.hip -- batches of gates on one device: the backend switch, the allocation rules around stream captures, device-pointer and
// host-pointer batches, MUX, the programmable-bootstrap entry points (their tables: rtfhe_lut.hip), synchronisation and the timers bench.py reads.
#include "rtfhe_host.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace rtfhe_host {

int backend_prepare(rtfhe_ctx* ctx) {
    if (ctx->backend == RTFHE_BACKEND_NTT_EXACT) return ntt_prepare(ctx);
    if (ctx->backend == RTFHE_BACKEND_FFT_SPLIT_EXACT) return xfft_prepare(ctx);
    return 0;
}

// Scratch is sized outside launches (hipMalloc is not allowed inside a stream capture).  Every step leaves b consistent: it is cleared before
// anything is freed, so a failure cannot leave a freed address behind, and a pair whose second hipMalloc fails gives the first back.
int grow_scratch(rtfhe_ctx* ctx, StreamScratch& b, const ScratchShape& shape, size_t need) {
    if (b.cap >= need) return 0;
    HIPCHECK(ctx, hipDeviceSynchronize());            // earlier launches may still read the old buffers
    const StreamScratch old = b;
    b = StreamScratch{};
    hipError_t e = hipSuccess;
    for (uint32_t* d : old.d) {
        if (!d) continue;
        if (old.captured) ctx->mux_retired.push_back(d);      // a caller's graph holds its address: kept until the context goes
        else if (hipError_t f = hipFree(d); e == hipSuccess) e = f;
    }
    const size_t cap = ((need < shape.min_cap ? shape.min_cap : need) + shape.tile - 1) / shape.tile * shape.tile;
    for (int i = 0; i < shape.bufs && e == hipSuccess; i++) e = hipMalloc((void**)&b.d[i], cap * shape.unit_bytes);
    if (e != hipSuccess) {
        for (uint32_t*& d : b.d) { if (d) (void)hipFree(d); d = nullptr; }
        return fail(ctx, RTFHE_ERR_HIP, std::string("per-stream scratch (hipFree / hipMalloc): ") + hipGetErrorString(e));
    }
    b.cap = cap;
    return 0;
}

int stream_scratch(rtfhe_ctx* ctx, ScratchMap& map, hipStream_t s, bool in_capture, const ScratchShape& shape, size_t need, const char* refusal,
                   StreamScratch*& out, StreamScratch* own) {
    out = own;
    if (!out) {
        auto it = map.find(s);
        if (it != map.end()) out = &it->second;
    }
    if (in_capture) {
        if (!out || out->cap < need) return fail(ctx, RTFHE_ERR_STATE, refusal);
        out->captured = true;
        return 0;
    }
    if (!out) out = &map[s];
    return grow_scratch(ctx, *out, shape, need);
}

int launch_bootstrap(rtfhe_ctx* ctx, int op, int mode, int steps, const void* d_in0, const void* d_in1, void* d_out,
                     size_t count, hipStream_t s, const int32_t* d_ops, const int32_t* d_idx0, const int32_t* d_idx1, const int32_t* d_idx_out, int32_t num_wires,
                     const LutRef& lut) {
    if (!ctx->has_bk) return fail(ctx, RTFHE_ERR_STATE, "bootstrapping key not loaded");
    if (mode == MODE_GATE && !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    if (count == 0) return 0;
    if (count > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    BootstrapArgs a{};
    a.tw = ctx->d_tw; a.bk = ctx->d_bk; a.ksk = ctx->d_ksk;
    a.in0 = (const uint32_t*)d_in0; a.in1 = (const uint32_t*)(d_in1 ? d_in1 : d_in0); a.out = (uint32_t*)d_out;
    a.count = (int)count; a.op = op; a.n = ctx->p.n; a.steps = steps; a.mode = mode; a.ksw = ctx->ksw;
    a.npad = (ctx->p.n + 1 + 63) / 64 * 64;
    a.ops = d_ops; a.idx0 = d_idx0; a.idx1 = d_idx1; a.idx_out = d_idx_out;
    a.num_wires = num_wires; a.fault = ctx->d_fault;
    a.dbg = ctx->d_dbg;
    a.ext = nullptr;
    struct Unset { bool& f; ~Unset() { f = false; } } unset{ctx->foreign_capture};
    // Whatever allocates happens here, outside any stream capture: the split path's sample buffer of this stream is created / grows, and the
    // second key layout the dispatch of this batch reads is built on first use.  Inside a capture that is not rtfhe_circuit_create's own
    // (which prepared both before it began) the batch stays on the fused kernel and on the kernels that read the canonical key layout.
    if (!ctx->tlwe1_capture) {
        if (capturing(s)) {
            ctx->foreign_capture = true;
        } else {
            if (int rc = ensure_bk_layouts(ctx, count, mode)) return rc;
            if (mode == MODE_GATE && ctx->ks_mm_min > 0 && ctx->d_ksmat)
                if (int rc = ensure_tlwe1(ctx, ctx->tlwe1[s], count)) return rc;
        }
    }
    if (lut.tv && ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "programmable bootstrapping runs on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR)");
    if (ctx->backend == RTFHE_BACKEND_NTT_EXACT) {
        if (int rc = ntt_prepare(ctx)) return rc;
        return launch_bootstrap_ntt(ctx, a, s);
    }
    if (ctx->backend == RTFHE_BACKEND_FFT_SPLIT_EXACT) {
        if (int rc = xfft_prepare(ctx)) return rc;
        return launch_bootstrap_xfft(ctx, a, s);
    }
    return launch_bootstrap_fft(ctx, a, s, lut);
}

int run_host_bootstrap_one(rtfhe_ctx* ctx, int op, int mode, int steps, const uint32_t* in0, const uint32_t* in1,
                                  uint32_t* out, size_t count, size_t out_words) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    const size_t in_bytes = count * ((size_t)ctx->p.n + 1) * 4, out_bytes = count * out_words * 4;
    if (int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, in_bytes)) return rc;
    if (int rc = ensure(ctx, &ctx->d_c, &ctx->cap_c, out_bytes)) return rc;
    if (int rc = copy_in(ctx, ctx->d_a, in0, in_bytes, 0)) return rc;
    const void* d1 = nullptr;
    if (in1) {
        if (int rc = ensure(ctx, &ctx->d_b, &ctx->cap_b, in_bytes)) return rc;
        if (int rc = copy_in(ctx, ctx->d_b, in1, in_bytes, 1)) return rc;
        d1 = ctx->d_b;
    }
    if (int rc = launch_bootstrap(ctx, op, mode, steps, ctx->d_a, d1, ctx->d_c, count, ctx->stream)) return rc;
    return copy_out(ctx, out, ctx->d_c, out_bytes, 2);
}

int run_host_pbs_one(rtfhe_ctx* ctx, const LutRef& lut, const int32_t* lut_idx, const uint32_t* in, uint32_t* out, size_t count) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    const size_t bytes = count * ((size_t)ctx->p.n + 1) * 4, out_bytes = lut.shift > 0 ? bytes << lut.shift : bytes;
    if (int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, bytes)) return rc;
    if (int rc = ensure(ctx, &ctx->d_c, &ctx->cap_c, out_bytes)) return rc;
    if (int rc = copy_in(ctx, ctx->d_a, in, bytes, 0)) return rc;
    LutRef l = lut;
    if (lut_idx) {      // the indices ride in the second operand's staging buffer (a bootstrap has one operand)
        if (int rc = ensure(ctx, &ctx->d_b, &ctx->cap_b, count * 4)) return rc;
        if (int rc = copy_in(ctx, ctx->d_b, lut_idx, count * 4, 1)) return rc;
        l.idx = (const int32_t*)ctx->d_b;
    }
    if (l.shift >= 0) {
        if (int rc = launch_pbs_many(ctx, l, ctx->d_a, ctx->d_c, count, ctx->stream)) return rc;
    } else if (int rc = launch_bootstrap(ctx, RTFHE_COPY, MODE_GATE, ctx->p.n, ctx->d_a, nullptr, ctx->d_c, count, ctx->stream, nullptr, nullptr, nullptr,
                                         nullptr, 0, l)) {
        return rc;
    }
    return copy_out(ctx, out, ctx->d_c, out_bytes, 2);
}

// Many-LUT PBS on one device (include/rtfhe.h: rtfhe_pbs_many_batch): the bootstrap kernels' many-LUT twins in MODE_EXTRACT write the 2^shift
// samples of every gate into this stream's sample buffer at batch-wide rows (gate << shift) + j, then ONE batch key switch of count << shift
// rows writes [count][2^shift][n+1] -- with the matrix form of the key as the split path does (into the zeroed output), else one wave per
// sample.  Outside a stream capture the sample buffer grows and the second key layout is built here; inside one nothing may be allocated: the
// sample buffer is rtfhe_lut_circuit_create's own (handed over through tlwe1_capture), or else this stream's, which must already hold
// count << shift samples -- an eager many-PBS of at least `count` gates and at least this many outputs on the stream first -- and is then kept
// for as long as the context lives (StreamScratch::captured).
int launch_pbs_many(rtfhe_ctx* ctx, const LutRef& lut, const void* d_in, void* d_out, size_t count, hipStream_t s, bool zero_out) {
    if (!ctx->has_bk) return fail(ctx, RTFHE_ERR_STATE, "bootstrapping key not loaded");
    if (!ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "programmable bootstrapping runs on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR)");
    if (count == 0) return 0;
    const size_t rows = count << lut.shift;
    if (rows > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count << log2(n_out) too large");
    const bool cap = capturing(s);
    if (!cap)
        if (int rc = ensure_bk_layouts(ctx, count, MODE_EXTRACT)) return rc;
    StreamScratch* buf = nullptr;
    if (int rc = stream_scratch(ctx, ctx->tlwe1, s, cap, tlwe1_shape(ctx), rows,
                                "a many-LUT PBS inside a stream capture needs this stream's sample buffer to exist already: run one eager "
                                "rtfhe_pbs_many_batch_dev of at least this many gates and outputs on the stream before capturing", buf, ctx->tlwe1_capture))
        return rc;
    BootstrapArgs a{};
    a.tw = ctx->d_tw; a.bk = ctx->d_bk; a.ksk = ctx->d_ksk;
    a.in0 = (const uint32_t*)d_in; a.in1 = a.in0; a.out = (uint32_t*)d_out;
    a.count = (int)count; a.op = RTFHE_COPY; a.n = ctx->p.n; a.steps = ctx->p.n; a.mode = MODE_EXTRACT; a.ksw = ctx->ksw;
    a.npad = (ctx->p.n + 1 + 63) / 64 * 64;
    a.fault = ctx->d_fault; a.dbg = ctx->d_dbg;
    a.ext = buf->d[0]; a.ext_first = 0;
    if (int rc = launch_bootstrap_fft(ctx, a, s, lut)) return rc;
    return launch_key_switch_rows(ctx, buf->d[0], (uint32_t*)d_out, rows, s, zero_out);
}

// hom_mux (tfhe.rs:27-40): i1 = AND(c, in1); i0 = AND(-c, in0); bootstrap(i1 + i0 + 1/8) -- the last line is hom_or(i1, i0).
// Three launches back to back on stream s with i1 / i0 kept in the context's own device buffers OF THAT STREAM (advisor r5: one pair shared by
// every stream let two overlapping MUX batches overwrite each other's intermediates).  Inside a caller's stream capture nothing may be
// allocated or synchronised: the call goes through only if this stream's pair already holds the batch (run one eager MUX batch of at least this
// size on the stream first) -- and that pair is then kept for as long as the context lives, because the graph owns its addresses.
int mux_dev_one(rtfhe_ctx* ctx, const void* d_c, const void* d_in0, const void* d_in1, void* d_out, size_t count, hipStream_t s) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    const size_t bytes = count * ((size_t)ctx->p.n + 1) * 4;
    StreamScratch* mb = nullptr;
    if (int rc = stream_scratch(ctx, ctx->mux, s, capturing(s), ScratchShape{2, 1}, bytes,
                                "a MUX batch inside a stream capture needs this stream's intermediate buffers to exist already: run one eager MUX batch of "
                                "at least this many gates on the stream before capturing", mb))
        return rc;
    void* const i1 = mb->d[0];
    void* const i0 = mb->d[1];
    const int n = ctx->p.n;
    if (int rc = launch_bootstrap(ctx, RTFHE_AND, MODE_GATE, n, d_c, d_in1, i1, count, s)) return rc;
    if (int rc = launch_bootstrap(ctx, RTFHE_ANDNY, MODE_GATE, n, d_c, d_in0, i0, count, s)) return rc;
    return launch_bootstrap(ctx, RTFHE_OR, MODE_GATE, n, i1, i0, d_out, count, s);
}

// ... with host buffers: one copy in (c, in0, in1), the three launches on the context's stream, one copy out
int mux_host_one(rtfhe_ctx* ctx, const uint32_t* c, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    const size_t bytes = count * ((size_t)ctx->p.n + 1) * 4;
    if (int rc = ensure(ctx, &ctx->d_a, &ctx->cap_a, bytes)) return rc;
    if (int rc = ensure(ctx, &ctx->d_b, &ctx->cap_b, bytes)) return rc;
    if (int rc = ensure(ctx, &ctx->d_c, &ctx->cap_c, bytes)) return rc;
    if (int rc = copy_in(ctx, ctx->d_a, c, bytes, 0)) return rc;
    if (int rc = copy_in(ctx, ctx->d_b, in1, bytes, 1)) return rc;
    if (int rc = copy_in(ctx, ctx->d_c, in0, bytes, 2)) return rc;
    if (int rc = mux_dev_one(ctx, ctx->d_a, ctx->d_c, ctx->d_b, ctx->d_a, count, ctx->stream)) return rc;      // (the OR writes d_a after both ANDs have read it: one stream)
    return copy_out(ctx, out, ctx->d_a, bytes, 0);
}

}  // namespace rtfhe_host

extern "C" {

// Device-pointer batches enqueue on the caller's stream and return without synchronising.  On a multi-device context the batch lives on the
// primary device and is sharded over all devices (rtfhe_multi.hip: sharded_dev_batch).
int rtfhe_gate_batch_dev(rtfhe_ctx* ctx, int op, const void* d_in0, const void* d_in1, void* d_out, size_t count, void* stream) {
    if (int rc = use(ctx)) return rc;
    if (op < RTFHE_NAND || op > RTFHE_ANDNY) return fail(ctx, RTFHE_ERR_INVALID, "unknown gate");
    if (!d_in0 || !d_out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (int rc = device_pointers(ctx, "rtfhe_gate_batch_dev", {d_in0, d_out}, {d_in1})) return rc;
    if (!ctx->peers.empty()) return sharded_dev_batch(ctx, op, nullptr, d_in0, d_in1, d_out, count, (hipStream_t)stream);
    return launch_bootstrap(ctx, op, MODE_GATE, ctx->p.n, d_in0, d_in1, d_out, count, (hipStream_t)stream);
}

int rtfhe_bootstrap_batch_dev(rtfhe_ctx* ctx, const void* d_tlwe, void* d_out, size_t count, void* stream) {
    return rtfhe_gate_batch_dev(ctx, RTFHE_COPY, d_tlwe, nullptr, d_out, count, stream);
}

int rtfhe_mux_batch_dev(rtfhe_ctx* ctx, const void* d_c, const void* d_in0, const void* d_in1, void* d_out, size_t count, void* stream) {
    if (int rc = use(ctx)) return rc;
    if (!d_c || !d_in0 || !d_in1 || !d_out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (int rc = device_pointers(ctx, "rtfhe_mux_batch_dev", {d_c, d_in0, d_in1, d_out})) return rc;
    if (!ctx->has_bk) return fail(ctx, RTFHE_ERR_STATE, "bootstrapping key not loaded");
    if (!ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    if (count > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    if (!ctx->peers.empty()) return sharded_dev_batch(ctx, -1, d_c, d_in0, d_in1, d_out, count, (hipStream_t)stream);
    return mux_dev_one(ctx, d_c, d_in0, d_in1, d_out, count, (hipStream_t)stream);
}

// ---- programmable bootstrapping (include/rtfhe.h; the tables themselves: rtfhe_lut.hip) ----
// what both PBS entries check before anything is launched
static int pbs_ready(rtfhe_ctx* ctx, const rtfhe_lut* lut) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = handles_ready(ctx, {ref(lut)})) return rc;
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "programmable bootstrapping runs on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); "
                                            "select it with rtfhe_set_backend");
    if (!ctx->has_bk) return fail(ctx, RTFHE_ERR_STATE, "bootstrapping key not loaded");
    if (!ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    return 0;
}

int rtfhe_pbs_batch(rtfhe_ctx* ctx, const rtfhe_lut* lut, const int32_t* lut_idx, const uint32_t* tlwe, uint32_t* out, size_t count) {
    if (int rc = pbs_ready(ctx, lut)) return rc;
    if (!tlwe || !out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (count > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    if (lut_idx)
        for (size_t g = 0; g < count; g++)
            if ((uint32_t)lut_idx[g] >= (uint32_t)lut->n_lut)
                return fail(ctx, RTFHE_ERR_INVALID, "lut_idx[" + std::to_string(g) + "] = " + std::to_string(lut_idx[g]) + " is outside [0, " + std::to_string(lut->n_lut) + ")");
    return sharded_host_pbs(ctx, lut, lut_idx, tlwe, out, count, pbs_shift(ctx, lut));      // encrypted or rounded: the many-LUT path, one output
}

int rtfhe_pbs_batch_dev(rtfhe_ctx* ctx, const rtfhe_lut* lut, const void* d_lut_idx, const void* d_tlwe, void* d_out, size_t count, void* stream) {
    if (int rc = pbs_ready(ctx, lut)) return rc;
    if (int rc = use(ctx)) return rc;
    if (!d_tlwe || !d_out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (int rc = device_pointers(ctx, "rtfhe_pbs_batch_dev", {d_tlwe, d_out}, {d_lut_idx})) return rc;
    if (count > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    if (pbs_shift(ctx, lut) == 0) {      // the many-LUT path with one output (MODE_EXTRACT, then the batch key switch): its capture rule applies
        if (!ctx->peers.empty())
            return sharded_dev_batch(ctx, RTFHE_COPY, nullptr, d_tlwe, nullptr, d_out, count, (hipStream_t)stream, lut, (const int32_t*)d_lut_idx, 0);
        return launch_pbs_many(ctx, lut_on(lut, 0, (const int32_t*)d_lut_idx, 0), d_tlwe, d_out, count, (hipStream_t)stream);
    }
    if (!ctx->peers.empty())
        return sharded_dev_batch(ctx, RTFHE_COPY, nullptr, d_tlwe, nullptr, d_out, count, (hipStream_t)stream, lut, (const int32_t*)d_lut_idx);
    return launch_bootstrap(ctx, RTFHE_COPY, MODE_GATE, ctx->p.n, d_tlwe, nullptr, d_out, count, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr, 0,
                            lut_on(lut, 0, (const int32_t*)d_lut_idx));
}

// ---- many-LUT PBS: 2^t outputs of one blind rotation (include/rtfhe.h) ----
static int many_shift(rtfhe_ctx* ctx, int32_t n_out, int32_t* shift) {
    for (int t = 0; t <= 3; t++)
        if (n_out == (1 << t)) { *shift = t; return 0; }
    return fail(ctx, RTFHE_ERR_INVALID, "n_out = " + std::to_string(n_out) + ": a many-LUT PBS gives 1, 2, 4 or 8 outputs per gate");
}

int rtfhe_pbs_many_batch(rtfhe_ctx* ctx, const rtfhe_lut* lut, int32_t n_out, const int32_t* lut_idx, const uint32_t* tlwe, uint32_t* out, size_t count) {
    if (int rc = pbs_ready(ctx, lut)) return rc;
    int32_t shift = 0;
    if (int rc = many_shift(ctx, n_out, &shift)) return rc;
    if (!tlwe || !out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (count > ((size_t)0x7fffffff >> shift)) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    if (lut_idx)
        for (size_t g = 0; g < count; g++)
            if ((uint32_t)lut_idx[g] >= (uint32_t)lut->n_lut)
                return fail(ctx, RTFHE_ERR_INVALID, "lut_idx[" + std::to_string(g) + "] = " + std::to_string(lut_idx[g]) + " is outside [0, " + std::to_string(lut->n_lut) + ")");
    return sharded_host_pbs(ctx, lut, lut_idx, tlwe, out, count, shift);
}

int rtfhe_pbs_many_batch_dev(rtfhe_ctx* ctx, const rtfhe_lut* lut, int32_t n_out, const void* d_lut_idx, const void* d_tlwe, void* d_out, size_t count,
                             void* stream) {
    if (int rc = pbs_ready(ctx, lut)) return rc;
    if (int rc = use(ctx)) return rc;
    int32_t shift = 0;
    if (int rc = many_shift(ctx, n_out, &shift)) return rc;
    if (!d_tlwe || !d_out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (int rc = device_pointers(ctx, "rtfhe_pbs_many_batch_dev", {d_tlwe, d_out}, {d_lut_idx})) return rc;
    if (count > ((size_t)0x7fffffff >> shift)) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    if (!ctx->peers.empty())
        return sharded_dev_batch(ctx, RTFHE_COPY, nullptr, d_tlwe, nullptr, d_out, count, (hipStream_t)stream, lut, (const int32_t*)d_lut_idx, shift);
    return launch_pbs_many(ctx, lut_on(lut, 0, (const int32_t*)d_lut_idx, shift), d_tlwe, d_out, count, (hipStream_t)stream);
}

int rtfhe_sync(rtfhe_ctx* ctx, void* stream) {
    if (int rc = use(ctx)) return rc;
    HIPCHECK(ctx, hipStreamSynchronize((hipStream_t)stream));
    // netlist waves validate their indices on the device; a skipped gate is reported here, once
    int32_t fault = 0;
    HIPCHECK(ctx, hipMemcpy(&fault, ctx->d_fault, 4, hipMemcpyDeviceToHost));
    if (fault) HIPCHECK(ctx, hipMemset(ctx->d_fault, 0, 4));
    // the peers' shares of a sharded programmable bootstrap check their table indices on their own devices (the caller's stream has waited for them)
    for (rtfhe_ctx* peer : ctx->peers) {
        int32_t f = 0;
        HIPCHECK(ctx, hipSetDevice(peer->device));
        HIPCHECK(ctx, hipMemcpy(&f, peer->d_fault, 4, hipMemcpyDeviceToHost));
        if (f) HIPCHECK(ctx, hipMemset(peer->d_fault, 0, 4));
        fault |= f;
    }
    HIPCHECK(ctx, hipSetDevice(ctx->device));
    if (fault) {
        return fail(ctx, RTFHE_ERR_INVALID, "netlist wave: wire index or opcode out of range, or programmable bootstrap: table index out of range "
                                            "(those gates were skipped)");
    }
    return 0;
}

int rtfhe_timer_begin(rtfhe_ctx* ctx, void* stream) {
    if (int rc = use(ctx)) return rc;
    ctx->launches = 0;
    ctx->timing = true;
    ctx->ks_events_used = 0;
    HIPCHECK(ctx, hipEventRecord(ctx->ev0, (hipStream_t)stream));
    return 0;
}

// total device time between begin and end, and of it the time inside the batch key switches of the split path (memset +
// k_key_switch_mm; 0 when every launch was the fused kernel): total - key_switch = the blind-rotation kernels (+ launch gaps)
int rtfhe_timer_end_detail(rtfhe_ctx* ctx, void* stream, double* ms, double* key_switch_ms, int64_t* launches) {
    if (int rc = use(ctx)) return rc;
    ctx->timing = false;
    HIPCHECK(ctx, hipEventRecord(ctx->ev1, (hipStream_t)stream));
    HIPCHECK(ctx, hipEventSynchronize(ctx->ev1));
    float f = 0.f;
    HIPCHECK(ctx, hipEventElapsedTime(&f, ctx->ev0, ctx->ev1));
    if (ms) *ms = (double)f;
    double ks = 0.0;
    for (size_t i = 0; i + 1 < ctx->ks_events_used; i += 2) {
        float g = 0.f;
        HIPCHECK(ctx, hipEventElapsedTime(&g, ctx->ks_events[i], ctx->ks_events[i + 1]));
        ks += (double)g;
    }
    ctx->ks_events_used = 0;
    if (key_switch_ms) *key_switch_ms = ks;
    if (launches) *launches = ctx->launches;
    return 0;
}

int rtfhe_timer_end(rtfhe_ctx* ctx, void* stream, double* ms, int64_t* launches) {
    return rtfhe_timer_end_detail(ctx, stream, ms, nullptr, launches);
}

int rtfhe_gate_batch(rtfhe_ctx* ctx, int op, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (op < RTFHE_NAND || op > RTFHE_ANDNY) return fail(ctx, RTFHE_ERR_INVALID, "unknown gate");
    const bool unary = (op == RTFHE_NOT || op == RTFHE_COPY);
    if (!unary && !in1) return fail(ctx, RTFHE_ERR_INVALID, "binary gate needs two inputs");
    return sharded_host_bootstrap(ctx, op, MODE_GATE, ctx->p.n, in0, unary ? nullptr : in1, out, count, (size_t)ctx->p.n + 1);
}

int rtfhe_bootstrap_batch(rtfhe_ctx* ctx, const uint32_t* tlwe, uint32_t* out, size_t count) {
    return rtfhe_gate_batch(ctx, RTFHE_COPY, tlwe, nullptr, out, count);
}

int rtfhe_blind_rotate_batch(rtfhe_ctx* ctx, const uint32_t* tlwe, int32_t steps, uint32_t* acc, size_t count) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (steps < 0 || steps > ctx->p.n) return fail(ctx, RTFHE_ERR_INVALID, "steps out of range");
    return sharded_host_bootstrap(ctx, RTFHE_COPY, MODE_BLIND_ROTATE, steps, tlwe, nullptr, acc, count, (size_t)2 * ctx->p.N);
}

int rtfhe_mux_batch(rtfhe_ctx* ctx, const uint32_t* c, const uint32_t* in0, const uint32_t* in1, uint32_t* out, size_t count) {
    if (int rc = use(ctx)) return rc;
    if (!c || !in0 || !in1 || !out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (!ctx->has_bk) return fail(ctx, RTFHE_ERR_STATE, "bootstrapping key not loaded");
    if (!ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    if (count > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count too large");
    return sharded_host_mux(ctx, c, in0, in1, out, count);
}

}  // extern "C"
