// rtfhe_compress.hip -- compressed results (include/rtfhe.h: rtfhe_tlwe_compress_batch_dev, rtfhe_trlwe_compress_batch_dev): result rows rounded to k
// bits per word and bit-packed on the device, in the stream of the computation that made them, so that only the small buffer leaves the GPU.  One
// kernel, k_compress_rows, serves both forms.  Nothing here reads a key or multiplies a polynomial: the calls work on every backend, allocate
// nothing and may be captured first thing on a fresh stream.  The argument checks and the key holder's CPU forms: rtfhe_compress_plan.cpp.
// The other direction (rtfhe_tlwe_expand_batch_dev, rtfhe_trlwe_expand_batch_dev): packed rows that came up from the host become full rows on
// the device, one kernel again, k_expand_rows, under the same contract and the same checks run with RTFHE_COMPRESS_EXPAND.
#include "rtfhe_host.hpp"

#include <algorithm>

#include "rtfhe_compress_plan.h"
#include "rtfhe_kernels_compress.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// `count` rows described by a (in, out, in_stride, seg, gat, L0, L, k, W) on stream s: one launch per slice [v0, v1) of a row's values, v0 a multiple
// of 32 and at most COMPRESS_COEF_MAX gathered values (idx[p0 ..]) in each -- one launch unless the coefficient list is longer than that
int launch_compress(rtfhe_ctx* ctx, CompressArgs a, const std::vector<int32_t>& idx, size_t count, hipStream_t s) {
    for (uint32_t v0 = 0; v0 < a.L;) {
        const uint32_t gather0 = std::max(v0, a.L0);
        const uint32_t v1 = a.L - gather0 > (uint32_t)COMPRESS_COEF_MAX ? (gather0 + COMPRESS_COEF_MAX) / 32 * 32 : a.L;
        a.w0 = v0 * a.k / 32; a.nw = (v1 * a.k + 31) / 32 - a.w0; a.p0 = gather0 - a.L0;
        a.total = (uint32_t)(count * a.nw);
        if (v1 > gather0) std::memcpy(a.coef, idx.data() + a.p0, (size_t)(v1 - gather0) * 4);
        if (int rc = launch_kernel(ctx, k_compress_rows, dim3((a.total + COMPRESS_THREADS - 1) / COMPRESS_THREADS), dim3(COMPRESS_THREADS), 0, s, a)) return rc;
        v0 = v1;
    }
    return 0;
}

// what both entry points do once their arguments have passed the host-only checks
int compress_dev(rtfhe_ctx* ctx, const char* name, const CompressArgs& a, const std::vector<int32_t>& idx, size_t count, void* stream) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, name, {a.out, a.in})) return rc;
    return launch_compress(ctx, a, idx, count, (hipStream_t)stream);
}

// ---- the other direction: packed rows expanded on the device (k_expand_rows) ----
// `count` rows described by a (in, out, W, out_stride, seg, L0, k, P, stride) on stream s.  inv == nullptr (lvl0 rows, a NULL list): one launch
// over the whole full row.  With a list, inv[0 .. N) its inverse map: the first launch owns the a polynomial and the last EXPAND_MAP_MAX words of
// b before it, each further launch the EXPAND_MAP_MAX words of b before that -- one launch at N = 1024, two at N = 2048.
int launch_expand(rtfhe_ctx* ctx, ExpandArgs a, const int16_t* inv, size_t count, hipStream_t s) {
    uint32_t o1 = a.out_stride;                                                    // this launch ends here
    uint32_t o0 = inv && a.seg > (uint32_t)EXPAND_MAP_MAX ? a.seg - EXPAND_MAP_MAX : 0u;
    for (;;) {
        a.o0 = a.j0 = o0; a.no = o1 - o0;
        a.total = (uint32_t)(count * a.no);                                        // count * out_stride < 2^32: rtfhe_trlwe_compress_plan's count * L < 2^31
        a.no_rcp = a.no > 1u ? (uint32_t)(((uint64_t)1 << 32) / a.no) : 0xFFFFFFFFu;
        if (inv) std::memcpy(a.inv, inv + o0, (size_t)(std::min(o1, a.seg) - o0) * sizeof(int16_t));      // the launch's words of b: at most EXPAND_MAP_MAX
        const uint64_t blocks = ((uint64_t)a.total + EXPAND_THREADS - 1) / EXPAND_THREADS;
        if (int rc = launch_kernel(ctx, k_expand_rows, dim3((unsigned)blocks), dim3(EXPAND_THREADS), 0, s, a)) return rc;
        if (o0 == 0) return 0;
        o1 = o0;
        o0 = o0 > (uint32_t)EXPAND_MAP_MAX ? o0 - EXPAND_MAP_MAX : 0u;
    }
}

int expand_dev(rtfhe_ctx* ctx, const char* name, const ExpandArgs& a, const int16_t* inv, size_t count, void* stream) {
    if (int rc = use(ctx)) return rc;
    if (count == 0) return 0;
    if (int rc = device_pointers(ctx, name, {a.out, a.in})) return rc;
    return launch_expand(ctx, a, inv, count, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int rtfhe_tlwe_compress_batch_dev(rtfhe_ctx* ctx, int32_t k, const void* d_tlwe, void* d_out, size_t count, void* stream) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    char err[256];
    if (int rc = rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_PACK, ctx->p.n, k, count, d_tlwe, d_out, err, sizeof err))
        return fail(ctx, rc, std::string("rtfhe_tlwe_compress_batch_dev: ") + err);
    CompressArgs a{};
    a.in = (const uint32_t*)d_tlwe; a.out = (uint32_t*)d_out;
    a.in_stride = a.L0 = a.L = (uint32_t)ctx->p.n + 1; a.k = (uint32_t)k; a.W = (uint32_t)rtfhe_compressed_words(a.L, k);
    return compress_dev(ctx, "rtfhe_tlwe_compress_batch_dev", a, {}, count, stream);
}

int rtfhe_trlwe_compress_batch_dev(rtfhe_ctx* ctx, int32_t k, const void* d_trlwe, int32_t P, const int32_t* coef, int32_t stride, void* d_out, size_t count,
                                   void* stream) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    const int32_t N = ctx->p.N;
    std::vector<int32_t> idx(P >= 1 && P <= N ? (size_t)P : 1, 0);
    char err[256];
    if (int rc = rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_PACK, N, k, P, coef, stride, count, d_trlwe, d_out, idx.data(), err, sizeof err))
        return fail(ctx, rc, std::string("rtfhe_trlwe_compress_batch_dev: ") + err);
    CompressArgs a{};
    a.in = (const uint32_t*)d_trlwe; a.out = (uint32_t*)d_out;
    a.in_stride = 2 * (uint32_t)N; a.seg = (uint32_t)N; a.gat = 0; a.L0 = (uint32_t)N; a.L = (uint32_t)(N + P); a.k = (uint32_t)k;
    a.W = (uint32_t)rtfhe_compressed_words(a.L, k);
    return compress_dev(ctx, "rtfhe_trlwe_compress_batch_dev", a, idx, count, stream);
}

int rtfhe_tlwe_expand_batch_dev(rtfhe_ctx* ctx, int32_t k, const void* d_words, void* d_tlwe, size_t count, void* stream) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    char err[256];
    if (int rc = rtfhe_tlwe_compress_plan(RTFHE_COMPRESS_EXPAND, ctx->p.n, k, count, d_words, d_tlwe, err, sizeof err))
        return fail(ctx, rc, std::string("rtfhe_tlwe_expand_batch_dev: ") + err);
    ExpandArgs a{};
    a.in = (const uint32_t*)d_words; a.out = (uint32_t*)d_tlwe;
    a.out_stride = a.L0 = (uint32_t)ctx->p.n + 1; a.seg = 0; a.k = (uint32_t)k; a.W = (uint32_t)rtfhe_compressed_words(a.L0, k);
    a.P = 0; a.stride = 1;                                                         // (no word of b: every lane has a value)
    return expand_dev(ctx, "rtfhe_tlwe_expand_batch_dev", a, nullptr, count, stream);
}

int rtfhe_trlwe_expand_batch_dev(rtfhe_ctx* ctx, int32_t k, const void* d_words, int32_t P, const int32_t* coef, int32_t stride, void* d_trlwe, size_t count,
                                 void* stream) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    const int32_t N = ctx->p.N;
    std::vector<int32_t> idx(P >= 1 && P <= N ? (size_t)P : 1, 0);
    char err[256];
    if (int rc = rtfhe_trlwe_compress_plan(RTFHE_COMPRESS_EXPAND, N, k, P, coef, stride, count, d_words, d_trlwe, idx.data(), err, sizeof err))
        return fail(ctx, rc, std::string("rtfhe_trlwe_expand_batch_dev: ") + err);
    ExpandArgs a{};
    a.in = (const uint32_t*)d_words; a.out = (uint32_t*)d_trlwe;
    a.out_stride = 2 * (uint32_t)N; a.seg = a.L0 = (uint32_t)N; a.k = (uint32_t)k; a.W = (uint32_t)rtfhe_compressed_words((size_t)N + (size_t)P, k);
    a.P = (uint32_t)P; a.stride = coef ? 0u : (uint32_t)stride;
    std::vector<int16_t> inv;
    if (coef) {
        inv.resize((size_t)N);
        if (rtfhe_expand_inverse_map(N, P, idx.data(), inv.data())) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_trlwe_expand_batch_dev: bad coefficient list");
    }
    return expand_dev(ctx, "rtfhe_trlwe_expand_batch_dev", a, coef ? inv.data() : nullptr, count, stream);
}

}  // extern "C"
