// rtfhe_extract.hip -- TRLWE sample extraction (include/rtfhe.h: rtfhe_trlwe_extract_batch[_dev], rtfhe_trlwe_extract_lvl1_batch[_dev]): chosen
// coefficients of TRLWEs that already exist, as lvl1 samples or -- through the extract tail every other entry point takes
// (launch_key_switch_rows) -- as lvl0 ciphertexts.  The inverse of the packing key switch (rtfhe_pack.hip).  Nothing here multiplies
// polynomials: the calls work on every backend and never read the bootstrapping key; the lvl1 form reads no key at all.
#include "rtfhe_host.hpp"

#include "rtfhe_extract_plan.h"
#include "rtfhe_kernels_extract.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// what every extract entry checks before anything is allocated or launched (the arguments themselves: rtfhe_extract_plan, host only); fills
// idx[P] with the coefficients (coef NULL: p * stride)
int extract_ready(rtfhe_ctx* ctx, const void* in, int32_t P, const int32_t* coef, int32_t stride, const void* out, size_t count, bool lvl1,
                  std::vector<int32_t>& idx) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    const int N = ctx->p.N;
    idx.assign(P >= 1 && P <= N ? (size_t)P : 1, 0);
    char err[256];
    if (int rc = rtfhe_extract_plan(N, P, coef, stride, count, in, out, (size_t)(lvl1 ? N : ctx->p.n) + 1, idx.data(), err, sizeof err)) return fail(ctx, rc, err);
    if (!lvl1 && !ctx->has_ksk) return fail(ctx, RTFHE_ERR_STATE, "key-switching key not loaded");
    return 0;
}

template <int LOGN>
int launch_extract_t(rtfhe_ctx* ctx, bool tiled, const TrlweExtractArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)(((size_t)a.M + 15) / 16)), block(64 * EXTRACT_WAVES);
    return tiled ? launch_kernel(ctx, k_trlwe_extract<LOGN, true>, grid, block, 0, s, a) : launch_kernel(ctx, k_trlwe_extract<LOGN, false>, grid, block, 0, s, a);
}

// `count` TRLWEs of P samples each on device buffers, primary device, stream s.  d_trlwe: [count][2][N]; d_out: [count * P][N+1] (lvl1), else
// [count * P][n+1] after the key switch of the samples in the stream's lvl1 sample buffer.
int launch_extract(rtfhe_ctx* ctx, const void* d_trlwe, int32_t P, const std::vector<int32_t>& idx, void* d_out, size_t count, bool lvl1, hipStream_t s) {
    if (count == 0) return 0;
    const size_t M = count * (size_t)P;
    StreamScratch* samples = nullptr;
    if (!lvl1) {
        const bool cap = capturing(s);
        const std::string refusal = !cap ? std::string()
                                         : "a TRLWE extraction inside a stream capture needs this stream's sample buffer to exist already: run one eager "
                                           "rtfhe_trlwe_extract_batch_dev of at least count * P = " + std::to_string(M) + " samples on the stream before capturing";
        if (int rc = stream_scratch(ctx, ctx->tlwe1, s, cap, tlwe1_shape(ctx), M, refusal.c_str(), samples, ctx->tlwe1_capture)) return rc;
    }
    TrlweExtractArgs a{};
    a.trlwe = (const uint32_t*)d_trlwe; a.out = lvl1 ? (uint32_t*)d_out : samples->d[0];
    a.M = (int32_t)M; a.P = P;
    for (int32_t p0 = 0; p0 < P; p0 += EXTRACT_COEF_MAX) {
        a.p0 = p0; a.np = P - p0 < EXTRACT_COEF_MAX ? P - p0 : EXTRACT_COEF_MAX;
        std::memcpy(a.coef, idx.data() + p0, (size_t)a.np * 4);
        if (int rc = ctx->logn == 11 ? launch_extract_t<11>(ctx, !lvl1, a, s) : launch_extract_t<10>(ctx, !lvl1, a, s)) return rc;
    }
    // identity_key_switch of the M samples, as the tree's extract form does it
    return lvl1 ? 0 : launch_key_switch_rows(ctx, samples->d[0], (uint32_t*)d_out, M, s);
}

int extract_dev(rtfhe_ctx* ctx, const void* d_trlwe, int32_t P, const int32_t* coef, int32_t stride, void* d_out, size_t count, bool lvl1, void* stream,
                const char* name) {
    std::vector<int32_t> idx;
    if (int rc = extract_ready(ctx, d_trlwe, P, coef, stride, d_out, count, lvl1, idx)) return rc;
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, name, {d_out, d_trlwe})) return rc;
    return launch_extract(ctx, d_trlwe, P, idx, d_out, count, lvl1, (hipStream_t)stream);
}

// host buffers: the rows ride in d_a, the result comes back through d_c (both grown to the call)
int extract_host(rtfhe_ctx* ctx, const uint32_t* trlwe, int32_t P, const int32_t* coef, int32_t stride, uint32_t* out, size_t count, bool lvl1) {
    std::vector<int32_t> idx;
    if (int rc = extract_ready(ctx, trlwe, P, coef, stride, out, count, lvl1, idx)) return rc;
    const size_t in_bytes = count * 2 * (size_t)ctx->p.N * 4, out_bytes = count * (size_t)P * ((size_t)(lvl1 ? ctx->p.N : ctx->p.n) + 1) * 4;
    return host_form(ctx, count, {staging_a(ctx), trlwe, in_bytes}, {staging_c(ctx), out, out_bytes, false}, {}, [&](const void* d_trlwe, const StagedIdx*, void* d_out) {
        return launch_extract(ctx, d_trlwe, P, idx, d_out, count, lvl1, ctx->stream);
    });
}

}  // namespace

extern "C" {

int rtfhe_trlwe_extract_batch(rtfhe_ctx* ctx, const uint32_t* trlwe, int32_t P, const int32_t* coef, int32_t stride, uint32_t* out, size_t count) {
    return extract_host(ctx, trlwe, P, coef, stride, out, count, false);
}

int rtfhe_trlwe_extract_batch_dev(rtfhe_ctx* ctx, const void* d_trlwe, int32_t P, const int32_t* coef, int32_t stride, void* d_out, size_t count,
                                  void* stream) {
    return extract_dev(ctx, d_trlwe, P, coef, stride, d_out, count, false, stream, "rtfhe_trlwe_extract_batch_dev");
}

int rtfhe_trlwe_extract_lvl1_batch(rtfhe_ctx* ctx, const uint32_t* trlwe, int32_t P, const int32_t* coef, int32_t stride, uint32_t* out, size_t count) {
    return extract_host(ctx, trlwe, P, coef, stride, out, count, true);
}

int rtfhe_trlwe_extract_lvl1_batch_dev(rtfhe_ctx* ctx, const void* d_trlwe, int32_t P, const int32_t* coef, int32_t stride, void* d_out, size_t count,
                                       void* stream) {
    return extract_dev(ctx, d_trlwe, P, coef, stride, d_out, count, true, stream, "rtfhe_trlwe_extract_lvl1_batch_dev");
}

}  // extern "C"
