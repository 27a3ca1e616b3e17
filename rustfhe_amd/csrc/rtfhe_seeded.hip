// rtfhe_seeded.hip -- seeded ciphertexts on the device (include/rtfhe.h: rtfhe_seeded_expand_dev, rtfhe_tlwe_seeded_expand_dev and the *_seeded
// upload calls): the one launch of k_seeded_expand (TRLWE rows) and of k_tlwe_seeded_expand (lvl0 rows), and the staging step the upload calls
// share -- the b halves go up through the context's staging buffer d_b (half the bytes of the unseeded upload) and are expanded into the buffer
// the unseeded twin copies its words into; from there on each upload call runs its twin's own code (the twins' units; rtfhe_load_ksk_seeded,
// whose b is one word per row, stages it beside rtfhe_load_ksk in rtfhe_context.hip).  The argument checks are host-only: rtfhe_seeded.cpp.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_seeded.hpp"
#include "rtfhe_kernels_tlwe_seeded.hpp"
#include "rtfhe_seeded_plan.h"

using namespace rtfhe;
using namespace rtfhe_host;

namespace rtfhe_host {

int seeded_ready(rtfhe_ctx* ctx, const char* name, int what, const void* seed, uint64_t first_row, const void* b, int group, const void* out, size_t rows) {
    char msg[200];
    if (int rc = rtfhe_seeded_plan(what, ctx->p.N, seed, first_row, b, group, out, rows, msg, sizeof(msg))) return fail(ctx, rc, std::string(name) + ": " + msg);
    return 0;
}

int launch_seeded_expand(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* d_b, int group, uint32_t* d_out, size_t rows, hipStream_t s) {
    if (rows == 0) return 0;
    SeededArgs a{};
    std::memcpy(a.seed, seed, sizeof(a.seed));
    a.first_row = first_row; a.b = d_b; a.out = d_out; a.blocks = (uint32_t)(rows * (size_t)(ctx->p.N / 16)); a.logn = ctx->logn; a.group = group;
    return launch_kernel(ctx, k_seeded_expand, dim3((a.blocks + SEEDED_THREADS - 1) / SEEDED_THREADS), dim3(SEEDED_THREADS), 0, s, a);
}

int stage_seeded(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* b, int group, size_t rows, void* d_full) {
    const size_t bytes = rows * (size_t)ctx->p.N * 4;
    if (int rc = ensure(ctx, &ctx->d_b, &ctx->cap_b, bytes)) return rc;
    if (int rc = copy_in(ctx, ctx->d_b, b, bytes, 1)) return rc;
    return launch_seeded_expand(ctx, seed, first_row, (const uint32_t*)ctx->d_b, group, (uint32_t*)d_full, rows, ctx->stream);
}

// ---- lvl0 rows: n mask words and one word of b (k_tlwe_seeded_expand) ----
int tlwe_seeded_ready(rtfhe_ctx* ctx, const char* name, int what, const void* seed, uint64_t first_row, const void* b, const void* out, size_t rows) {
    char msg[200];
    if (int rc = rtfhe_tlwe_seeded_plan(what, ctx->p.n, seed, first_row, b, out, rows, msg, sizeof(msg))) return fail(ctx, rc, std::string(name) + ": " + msg);
    return 0;
}

int launch_tlwe_seeded_expand(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* d_b, uint32_t* d_out, size_t stride, size_t rows,
                              hipStream_t s) {
    TlweSeededArgs a{};
    std::memcpy(a.seed, seed, sizeof(a.seed));
    a.first_row = first_row; a.b = d_b; a.out = d_out; a.n = (uint32_t)ctx->p.n; a.nb = (a.n + 15) / 16; a.blocks = (uint32_t)(rows * (size_t)a.nb);
    a.stride = (uint32_t)stride;
    return launch_kernel(ctx, k_tlwe_seeded_expand, dim3((a.blocks + TLWE_SEEDED_THREADS - 1) / TLWE_SEEDED_THREADS), dim3(TLWE_SEEDED_THREADS), 0, s, a);
}

}  // namespace rtfhe_host

extern "C" {

int rtfhe_seeded_expand_dev(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const void* d_b, int32_t group, void* d_out, size_t rows, void* stream) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = seeded_ready(ctx, "rtfhe_seeded_expand_dev", RTFHE_SEEDED_DEVICE, seed, first_row, d_b, group, d_out, rows)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, "rtfhe_seeded_expand_dev", {d_out, d_b})) return rc;
    return launch_seeded_expand(ctx, seed, first_row, (const uint32_t*)d_b, group, (uint32_t*)d_out, rows, (hipStream_t)stream);
}

int rtfhe_tlwe_seeded_expand_dev(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const void* d_b, void* d_out, size_t rows, void* stream) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = tlwe_seeded_ready(ctx, "rtfhe_tlwe_seeded_expand_dev", RTFHE_TLWE_SEEDED_DEVICE, seed, first_row, d_b, d_out, rows)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, "rtfhe_tlwe_seeded_expand_dev", {d_out, d_b})) return rc;
    return launch_tlwe_seeded_expand(ctx, seed, first_row, (const uint32_t*)d_b, (uint32_t*)d_out, (size_t)ctx->p.n + 1, rows, (hipStream_t)stream);
}

}  // extern "C"
