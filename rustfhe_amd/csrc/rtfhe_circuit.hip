// rtfhe_circuit.hip -- levelised netlists (BASELINE config 4): one dependency wave per call, or every wave of a netlist recorded once into a
// HIP graph and replayed as one submission.  Replaces eval_logic_expr over impl Logip for TFHE (nander/src/lib.rs:40-89).  LUT circuits
// (rtfhe_lut_circuit_create): netlists of many-LUT bootstraps of weighted wire sums, recorded the same way.
#include "rtfhe_host.hpp"
#include "rtfhe_kernels_lutc.hpp"

#include <algorithm>

using namespace rtfhe;
using namespace rtfhe_host;

namespace rtfhe_host {

// releases the graph objects of a circuit (the handle itself stays valid for rtfhe_circuit_destroy)
void circuit_release(rtfhe_circuit* c) {
    (void)hipSetDevice(c->device);
    if (c->exec) (void)hipGraphExecDestroy(c->exec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    if (c->d_samples) (void)hipFree(c->d_samples);
    for (void* d : c->d_owned) (void)hipFree(d);
    c->exec = nullptr; c->graph = nullptr; c->d_samples = nullptr; c->d_owned.clear();
}

// a circuit's own device buffers: listed in d_owned as they are allocated, so that circuit_release frees the ones that exist
int circuit_own(rtfhe_ctx* ctx, rtfhe_circuit* c, const char* name, std::initializer_list<std::pair<void**, size_t>> bufs) {
    for (const auto& [pp, bytes] : bufs) {
        if (hipMalloc(pp, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, RTFHE_ERR_HIP, std::string(name) + ": hipMalloc"); }
        c->d_owned.push_back(*pp);
    }
    return 0;
}

int circuit_fill(rtfhe_ctx* ctx, const char* name, void* d_desc, const std::vector<int32_t>& desc, void* d_tv, const rtfhe_lut* lut, void* d_zero, size_t zero_bytes) {
    if (hipMemcpy(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_tv, lut->d_tv[0], lut_bytes(ctx, lut), hipMemcpyDeviceToDevice) != hipSuccess || hipMemset(d_zero, 0, zero_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, RTFHE_ERR_HIP, std::string(name) + ": hipMemcpy / hipMemset");
    }
    return 0;
}

// The recorder's rule.  Nothing but kernel launches may happen inside the capture, so whatever allocates or synchronises is the
// caller's business before it calls.  Once the capture has begun there is no return before it has ended: enqueue's failure is kept and reported
// first, then the capture's.  tlwe1_capture is never left set, and the launches enqueue counted leave the context's counter whether it failed
// or not: a replay adds them (rtfhe_circuit_launch), the recording adds nothing.  On every failure c goes with this function's return
// (CircuitDrop), no context lists it and *out stays as the caller set it: null.
int circuit_record(rtfhe_ctx* ctx, NewCircuit c, StreamScratch* capture_samples, rtfhe_circuit** out, const std::function<int()>& enqueue) {
    const auto hip_fail = [&](const char* call, hipError_t e) { return fail(ctx, RTFHE_ERR_HIP, std::string(call) + ": " + hipGetErrorString(e)); };
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail("hipStreamSynchronize", e);
    e = hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) return hip_fail("hipStreamBeginCapture", e);
    const int64_t before = ctx->launches;
    ctx->tlwe1_capture = capture_samples;
    const int rc = enqueue();
    ctx->tlwe1_capture = nullptr;
    e = hipStreamEndCapture(ctx->stream, &c->graph);
    c->launches = ctx->launches - before;
    ctx->launches = before;
    if (rc) return rc;
    if (e != hipSuccess) return hip_fail("hipStreamEndCapture", e);
    e = hipGraphInstantiate(&c->exec, c->graph, nullptr, nullptr, 0);
    if (e != hipSuccess) return hip_fail("hipGraphInstantiate", e);
    ctx->circuits.push_back(c.get());
    *out = c.release();
    return 0;
}

// ---- LUT circuits: the gather / scatter launches around a wave's many-LUT PBS (a wave per node / per output row, LUTC_WAVES waves per workgroup) ----
namespace {

template <int F>
int launch_lut_gather_f(rtfhe_ctx* ctx, bool vec, const LutGatherArgs& a, hipStream_t s) {
    const dim3 grid((a.count + LUTC_WAVES - 1) / LUTC_WAVES), block(64 * LUTC_WAVES);
    return vec ? launch_kernel(ctx, k_lut_gather<F, true>, grid, block, 0, s, a) : launch_kernel(ctx, k_lut_gather<F, false>, grid, block, 0, s, a);
}

int launch_lut_gather(rtfhe_ctx* ctx, int fan_in, bool vec, const LutGatherArgs& a, hipStream_t s) {
    switch (fan_in) {
        case 1: return launch_lut_gather_f<1>(ctx, vec, a, s);
        case 2: return launch_lut_gather_f<2>(ctx, vec, a, s);
        case 3: return launch_lut_gather_f<3>(ctx, vec, a, s);
        case 4: return launch_lut_gather_f<4>(ctx, vec, a, s);
        case 5: return launch_lut_gather_f<5>(ctx, vec, a, s);
        case 6: return launch_lut_gather_f<6>(ctx, vec, a, s);
        case 7: return launch_lut_gather_f<7>(ctx, vec, a, s);
        case 8: return launch_lut_gather_f<8>(ctx, vec, a, s);
        default: return fail(ctx, RTFHE_ERR_INVALID, "fan_in out of range");
    }
}

int launch_lut_scatter(rtfhe_ctx* ctx, bool vec, const LutScatterArgs& a, hipStream_t s) {
    const dim3 grid((a.rows + LUTC_WAVES - 1) / LUTC_WAVES), block(64 * LUTC_WAVES);
    return vec ? launch_kernel(ctx, k_lut_scatter<true>, grid, block, 0, s, a) : launch_kernel(ctx, k_lut_scatter<false>, grid, block, 0, s, a);
}

std::string at(int32_t w, int64_t g) { return "wave " + std::to_string(w) + ", node " + std::to_string(g) + ": "; }

}  // namespace

}  // namespace rtfhe_host

extern "C" {

int rtfhe_circuit_wave_dev(rtfhe_ctx* ctx, const void* d_ops, const void* d_idx0, const void* d_idx1, const void* d_idx_out,
                           void* d_wires, size_t num_wires, size_t count, void* stream) {
    if (int rc = use(ctx)) return rc;
    if (!d_ops || !d_idx0 || !d_idx1 || !d_idx_out || !d_wires) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (num_wires == 0 || num_wires > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "num_wires out of range");
    if (int rc = device_pointers(ctx, "rtfhe_circuit_wave_dev", {d_ops, d_idx0, d_idx1, d_idx_out, d_wires})) return rc;
    return launch_bootstrap(ctx, RTFHE_COPY, MODE_GATE, ctx->p.n, d_wires, d_wires, d_wires, count, (hipStream_t)stream,
                            (const int32_t*)d_ops, (const int32_t*)d_idx0, (const int32_t*)d_idx1, (const int32_t*)d_idx_out,
                            (int32_t)num_wires);
}

// ---- a whole levelised netlist as ONE submission: its dependency waves captured once into a HIP graph, replayed per run ----
int rtfhe_circuit_create(rtfhe_ctx* ctx, const void* d_ops, const void* d_idx0, const void* d_idx1, const void* d_idx_out,
                         const int32_t* wave_offsets, int32_t num_waves, void* d_wires, size_t num_wires, rtfhe_circuit** out) {
    if (int rc = use(ctx)) return rc;
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!d_ops || !d_idx0 || !d_idx1 || !d_idx_out || !d_wires || !wave_offsets) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (num_waves < 1 || num_wires == 0 || num_wires > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "num_waves / num_wires out of range");
    for (int32_t w = 0; w < num_waves; w++)
        if (wave_offsets[w] < 0 || wave_offsets[w + 1] <= wave_offsets[w]) return fail(ctx, RTFHE_ERR_INVALID, "wave_offsets must be strictly increasing from >= 0");
    if (!ctx->has_bk || !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "keys not loaded");
    if (int rc = device_pointers(ctx, "rtfhe_circuit_create", {d_ops, d_idx0, d_idx1, d_idx_out, d_wires})) return rc;
    if (int rc = backend_prepare(ctx)) return rc;          // nothing but kernel launches may happen inside the capture
    for (int32_t w = 0; w < num_waves; w++)                // ... so the key layouts the waves' dispatches read are built now
        if (int rc = ensure_bk_layouts(ctx, (size_t)(wave_offsets[w + 1] - wave_offsets[w]), MODE_GATE)) return rc;
    NewCircuit c(new (std::nothrow) rtfhe_circuit());
    if (!c) return fail(ctx, RTFHE_ERR_NOMEM, "out of host memory");
    c->ctx = ctx; c->device = ctx->device; c->waves = num_waves; c->backend = ctx->backend;
    StreamScratch cbuf;                                 // ... so the circuit's own sample buffer (split path) is allocated now
    if (ctx->ks_mm_min > 0 && ctx->d_ksmat) {
        size_t widest = 0;
        for (int32_t w = 0; w < num_waves; w++) widest = std::max(widest, (size_t)(wave_offsets[w + 1] - wave_offsets[w]));
        if (int rc = ensure_tlwe1(ctx, cbuf, widest)) return rc;
        c->d_samples = cbuf.d[0];
    }
    // recorded by circuit_record, under its rule; no sample buffer, no split path: split_ok and the key switch's timer bracketing read tlwe1_capture
    return circuit_record(ctx, std::move(c), cbuf.d[0] ? &cbuf : nullptr, out, [&] {
        int rc = 0;
        for (int32_t w = 0; w < num_waves && !rc; w++) {
            const size_t off = (size_t)wave_offsets[w], cnt = (size_t)(wave_offsets[w + 1] - wave_offsets[w]);
            rc = launch_bootstrap(ctx, RTFHE_COPY, MODE_GATE, ctx->p.n, d_wires, d_wires, d_wires, cnt, ctx->stream,
                                  (const int32_t*)d_ops + off, (const int32_t*)d_idx0 + off, (const int32_t*)d_idx1 + off,
                                  (const int32_t*)d_idx_out + off, (int32_t)num_wires);
        }
        return rc;
    });
}

// ---- a LUT circuit: waves of "weighted sum of wires, then a many-LUT PBS", recorded like rtfhe_circuit_create ----
int rtfhe_lut_circuit_create(rtfhe_ctx* ctx, const rtfhe_lut* lut, int32_t fan_in, const int32_t* in_idx, const int32_t* weights, const uint32_t* cst,
                             const int32_t* lut_idx, const int32_t* wave_offsets, const int32_t* wave_n_out, int32_t num_waves, const int32_t* out_idx,
                             void* d_wires, size_t num_wires, rtfhe_circuit** out) {
    if (int rc = use(ctx)) return rc;
    if (!out) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = handles_ready(ctx, {ref(lut)})) return rc;
    if (ctx->backend != RTFHE_BACKEND_FFT64_MIRROR)
        return fail(ctx, RTFHE_ERR_INVALID, "LUT circuits (programmable bootstrapping) run on the FP64 mirror backend only (RTFHE_BACKEND_FFT64_MIRROR); "
                                            "select it with rtfhe_set_backend");
    if (!in_idx || !weights || !wave_offsets || !wave_n_out || !out_idx || !d_wires) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (fan_in < 1 || fan_in > 8) return fail(ctx, RTFHE_ERR_INVALID, "fan_in = " + std::to_string(fan_in) + " is outside [1, 8]");
    if (num_waves < 1 || num_wires == 0 || num_wires > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "num_waves / num_wires out of range");
    // the whole description is checked before anything is allocated, captured or launched
    const int32_t nw = (int32_t)num_wires;
    std::vector<int32_t> written(num_wires, -1);          // the wave that last wrote each wire
    std::vector<int32_t> out_base(num_waves + 1, 0);      // first row of each wave in out_idx
    size_t widest = 0, widest_rows = 0;
    for (int32_t w = 0; w < num_waves; w++) {
        if (wave_offsets[w] < 0 || wave_offsets[w + 1] <= wave_offsets[w])
            return fail(ctx, RTFHE_ERR_INVALID, "wave " + std::to_string(w) + ": wave_offsets must be strictly increasing from >= 0");
        const int32_t th = wave_n_out[w];
        if (th != 1 && th != 2 && th != 4 && th != 8)
            return fail(ctx, RTFHE_ERR_INVALID, "wave " + std::to_string(w) + ": n_out = " + std::to_string(th) + ": a many-LUT PBS gives 1, 2, 4 or 8 outputs per node");
        const size_t cnt = (size_t)(wave_offsets[w + 1] - wave_offsets[w]);
        if ((size_t)out_base[w] + cnt * th > 0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "wave " + std::to_string(w) + ": too many output rows");
        out_base[w + 1] = out_base[w] + (int32_t)(cnt * th);
        widest = std::max(widest, cnt);
        widest_rows = std::max(widest_rows, cnt * th);
        for (int32_t g = wave_offsets[w]; g < wave_offsets[w + 1]; g++) {
            for (int32_t k = 0; k < fan_in; k++) {
                const int32_t i = in_idx[(size_t)g * fan_in + k];
                if (i < -1 || i >= nw)
                    return fail(ctx, RTFHE_ERR_INVALID, at(w, g) + "in_idx[" + std::to_string(g) + "][" + std::to_string(k) + "] = " + std::to_string(i) +
                                                        " is outside [-1, num_wires)");
            }
            if (lut_idx && (uint32_t)lut_idx[g] >= (uint32_t)lut->n_lut)
                return fail(ctx, RTFHE_ERR_INVALID, at(w, g) + "lut_idx[" + std::to_string(g) + "] = " + std::to_string(lut_idx[g]) + " is outside [0, " +
                                                    std::to_string(lut->n_lut) + ")");
            for (int32_t j = 0; j < th; j++) {
                const size_t r = (size_t)out_base[w] + (size_t)(g - wave_offsets[w]) * th + j;
                const int32_t o = out_idx[r];
                if (o < 0 || o >= nw)
                    return fail(ctx, RTFHE_ERR_INVALID, at(w, g) + "out_idx[" + std::to_string(r) + "] = " + std::to_string(o) + " is outside [0, num_wires)");
                if (written[o] == w) return fail(ctx, RTFHE_ERR_INVALID, at(w, g) + "wire " + std::to_string(o) + " is written twice in this wave");
                written[o] = w;
            }
        }
    }
    if (!ctx->has_bk || !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "keys not loaded");
    if (int rc = device_pointers(ctx, "rtfhe_lut_circuit_create", {d_wires})) return rc;
    // everything that allocates or synchronises happens now, outside the capture: the key layouts the waves' dispatches read, the sample buffer,
    // the circuit's own copies of the description and the table rows, the gathered inputs and the key-switched outputs
    for (int32_t w = 0; w < num_waves; w++)
        if (int rc = ensure_bk_layouts(ctx, (size_t)(wave_offsets[w + 1] - wave_offsets[w]), MODE_EXTRACT)) return rc;
    const int32_t first = wave_offsets[0], nodes = wave_offsets[num_waves] - first, rows = out_base[num_waves];
    const size_t n1 = (size_t)ctx->p.n + 1;
    NewCircuit c(new (std::nothrow) rtfhe_circuit());
    if (!c) return fail(ctx, RTFHE_ERR_NOMEM, "out of host memory");
    c->ctx = ctx; c->device = ctx->device; c->waves = num_waves; c->backend = ctx->backend;
    StreamScratch cbuf;
    if (int rc = ensure_tlwe1(ctx, cbuf, widest_rows)) return rc;
    c->d_samples = cbuf.d[0];
    // description: in_idx, weights [nodes][fan_in] | cst, lut_idx [nodes] | out_idx [rows]
    const size_t desc_words = (size_t)nodes * (2 * fan_in + 2) + rows;
    std::vector<int32_t> desc(desc_words, 0);
    int32_t* h_in = desc.data();
    int32_t* h_wt = h_in + (size_t)nodes * fan_in;
    int32_t* h_cst = h_wt + (size_t)nodes * fan_in;
    int32_t* h_lut = h_cst + nodes;
    int32_t* h_out = h_lut + nodes;
    std::memcpy(h_in, in_idx + (size_t)first * fan_in, (size_t)nodes * fan_in * 4);
    std::memcpy(h_wt, weights + (size_t)first * fan_in, (size_t)nodes * fan_in * 4);
    if (cst) std::memcpy(h_cst, cst + first, (size_t)nodes * 4);
    if (lut_idx) std::memcpy(h_lut, lut_idx + first, (size_t)nodes * 4);
    std::memcpy(h_out, out_idx, (size_t)rows * 4);
    void *d_desc = nullptr, *d_gather = nullptr, *d_ks = nullptr, *d_tv = nullptr;
    if (int rc = circuit_own(ctx, c.get(), "rtfhe_lut_circuit_create",
                             {{&d_desc, desc_words * 4}, {&d_gather, widest * n1 * 4}, {&d_ks, widest_rows * n1 * 4}, {&d_tv, lut_bytes(ctx, lut)}})) return rc;
    if (int rc = circuit_fill(ctx, "rtfhe_lut_circuit_create", d_desc, desc, d_tv, lut, d_ks, widest_rows * n1 * 4)) return rc;
    const int32_t* d_in = (const int32_t*)d_desc;
    const int32_t* d_wt = d_in + (size_t)nodes * fan_in;
    const uint32_t* d_cst = (const uint32_t*)(d_wt + (size_t)nodes * fan_in);
    const int32_t* d_lut = (const int32_t*)d_cst + nodes;
    const int32_t* d_out = d_lut + nodes;
    const bool vec = n1 % 4 == 0 && (uintptr_t)d_wires % 16 == 0;      // (the circuit's own buffers come from hipMalloc)
    // recorded by circuit_record, under its rule
    return circuit_record(ctx, std::move(c), &cbuf, out, [&] {
        int rc = 0;
        for (int32_t w = 0; w < num_waves && !rc; w++) {
            const int32_t off = wave_offsets[w] - first, cnt = wave_offsets[w + 1] - wave_offsets[w], th = wave_n_out[w];
            const int32_t shift = th == 1 ? 0 : th == 2 ? 1 : th == 4 ? 2 : 3;
            const LutGatherArgs ga{(const uint32_t*)d_wires, (uint32_t*)d_gather, d_in + (size_t)off * fan_in, d_wt + (size_t)off * fan_in, d_cst + off, cnt,
                                   (int32_t)n1, nw};
            rc = launch_lut_gather(ctx, fan_in, vec, ga, ctx->stream);
            if (!rc) rc = launch_pbs_many(ctx, LutRef{(const uint32_t*)d_tv, lut_idx ? d_lut + off : nullptr, lut->n_lut, shift, lut->encrypted, ctx->decomp == RTFHE_DECOMP_ROUNDED}, d_gather, d_ks, (size_t)cnt,
                                          ctx->stream, false);      // (d_ks is zero: cleared at creation and by every scatter, no memset node)
            const LutScatterArgs sa{(uint32_t*)d_ks, (uint32_t*)d_wires, d_out + out_base[w], cnt * th, (int32_t)n1, nw};
            if (!rc) rc = launch_lut_scatter(ctx, vec, sa, ctx->stream);
        }
        return rc;
    });
}

int rtfhe_circuit_launch(rtfhe_circuit* c, void* stream) {
    if (!c) return fail(nullptr, RTFHE_ERR_INVALID, "null circuit");
    if (!c->ctx) return fail(nullptr, RTFHE_ERR_STATE, "the circuit's context has been destroyed");
    rtfhe_ctx* ctx = c->ctx;
    if (int rc = use(ctx)) return rc;
    if (c->stale) return fail(ctx, RTFHE_ERR_STATE, "the circuit was recorded on an exact backend and the bootstrapping key has since been replaced by one without a "
                                                  "torus form (rtfhe_load_bk_fft): its key form could not follow; record the circuit again");
    if (c->sel_gone) return fail(ctx, RTFHE_ERR_STATE, "the selector set (rtfhe_trgsw) this CMUX netlist was recorded on has been destroyed: its graph reads the "
                                                     "set's spectra in place; record the circuit again on a live set");
    HIPCHECK(ctx, hipGraphLaunch(c->exec, (hipStream_t)stream));
    ctx->launches += c->launches;
    return 0;
}

void rtfhe_circuit_destroy(rtfhe_circuit* c) { handle_destroy(&rtfhe_ctx::circuits, c, circuit_release); }

}  // extern "C"
