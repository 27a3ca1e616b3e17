// rtfhe_pack.hip -- the packing key switch (include/rtfhe.h: rtfhe_packing_key_create, rtfhe_pack_batch[_dev]): packing keys as signed byte
// limbs in operand order (k_pkmat_build), the stream's buffer of key-switched samples and the rules around stream
// captures, k_pack_ks_mm then k_pack_combine per call.  (Its rows go into an encrypted table through rtfhe_lut_update_dev, rtfhe_lut.hip.)
// Nothing here multiplies polynomials: the calls work on every backend and never read the bootstrapping key.
#include "rtfhe_host.hpp"

#include "rtfhe_extract_plan.h"
#include "rtfhe_kernels_pack.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// what both pack entries check before anything is allocated or launched: the handle, then the arguments themselves (rtfhe_pack_plan, host only);
// fills shift[P] with the positions (pos NULL: p * rep)
int pack_ready(rtfhe_ctx* ctx, const rtfhe_packing_key* pk, const void* in, int32_t P, const int32_t* pos, int32_t rep, const void* out, size_t count,
               std::vector<int32_t>& shift) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (int rc = handles_ready(ctx, {ref(pk)})) return rc;
    const int N = ctx->p.N;
    shift.assign(P >= 1 && P <= N ? (size_t)P : 1, 0);
    char err[256];
    if (int rc = rtfhe_pack_plan(N, P, pos, rep, count, in, out, shift.data(), err, sizeof err)) return fail(ctx, rc, err);
    return 0;
}

template <int LOGN>
int launch_combine_t(rtfhe_ctx* ctx, const PackCombineArgs& a, size_t count, hipStream_t s) {
    return launch_kernel(ctx, k_pack_combine<LOGN>, dim3((unsigned)(2 * count)), dim3(PACK_CT), 0, s, a);
}

// `count` outputs of P samples each on device buffers, primary device, stream s.  d_tlwe: [count * P][n+1], d_out: [count][2][N].
int launch_pack(rtfhe_ctx* ctx, const rtfhe_packing_key* pk, const void* d_tlwe, int32_t P, const std::vector<int32_t>& shift, int32_t rep, void* d_out,
                size_t count, hipStream_t s) {
    if (count == 0) return 0;
    const size_t N = (size_t)ctx->p.N, M = count * (size_t)P;
    const bool cap = capturing(s);
    const std::string refusal = !cap ? std::string()
                                     : "a packing key switch inside a stream capture needs this stream's sample buffer to exist already: run one eager "
                                       "rtfhe_pack_batch_dev of at least count * P = " + std::to_string(M) + " samples on the stream before capturing";
    StreamScratch* pb = nullptr;
    if (int rc = stream_scratch(ctx, ctx->pack, s, cap, ScratchShape{1, 2 * N * 4}, M, refusal.c_str(), pb)) return rc;
    uint32_t* d_s = pb->d[0];
    PackMmArgs m{};
    m.tlwe = (const uint32_t*)d_tlwe; m.kmat = pk->d_kmat; m.s = d_s;
    m.M = (int32_t)M; m.n = ctx->p.n; m.n16 = pk->n16; m.colgroups = pk->colgroups;
    m.mgroups = (int32_t)((M + 64 * PACK_WAVES - 1) / (64 * PACK_WAVES));
    if (int rc = launch_kernel(ctx, k_pack_ks_mm<8, 2>, dim3((unsigned)(m.colgroups * m.mgroups)), dim3(64 * PACK_WAVES), 0, s, m)) return rc;
    PackCombineArgs c{};
    c.s = d_s; c.tlwe = (const uint32_t*)d_tlwe; c.out = (uint32_t*)d_out;
    c.P = P; c.n = ctx->p.n; c.rep = rep;
    for (int32_t p0 = 0; p0 < P; p0 += PACK_POS_MAX) {
        c.p0 = p0; c.np = P - p0 < PACK_POS_MAX ? P - p0 : PACK_POS_MAX; c.accumulate = p0 ? 1 : 0;
        std::memcpy(c.pos, shift.data() + p0, (size_t)c.np * 4);
        if (int rc = ctx->logn == 11 ? launch_combine_t<11>(ctx, c, count, s) : launch_combine_t<10>(ctx, c, count, s)) return rc;
    }
    return 0;
}

}  // namespace

namespace rtfhe_host {

void packing_key_release(rtfhe_packing_key* k) {
    (void)hipSetDevice(k->ctx->device);
    if (k->d_kmat) (void)hipFree(k->d_kmat);
    k->d_kmat = nullptr;
}

}  // namespace rtfhe_host

// (args_ok: the caller's pointers; fill(d_raw, rows, raw_bytes) brings the key's rows into d_raw, done when it returns: the caller's copy, or a seeded
// key's expansion)
template <typename Fill>
static int packing_key_create_filled(rtfhe_ctx* ctx, bool args_ok, rtfhe_packing_key** out, Fill fill) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!args_ok) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_packing_key_create: null argument");
    *out = nullptr;
    if (ctx->p.ks_t != 8 || ctx->p.ks_basebit != 2)
        return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_packing_key_create: the packing key switch needs ks_t = 8 and ks_basebit = 2");
    if (int rc = use(ctx)) return rc;
    const size_t n = (size_t)ctx->p.n, N = (size_t)ctx->p.N, rows = n * 8 * 3, raw_bytes = rows * 2 * N * 4;
    NewHandle<rtfhe_packing_key> k = new_handle(ctx, packing_key_release);
    k->n16 = (int32_t)((n + 15) / 16 * 16);
    k->colgroups = (int32_t)(2 * N / 16);
    const size_t kmat_v4 = (size_t)k->colgroups * (k->n16 / 2) * 4 * 64;
    uint32_t* d_raw = nullptr;
    int rc = 0;
    if (hipMalloc((void**)&d_raw, raw_bytes) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_packing_key_create: hipMalloc (raw rows)");
    if (!rc && hipMalloc((void**)&k->d_kmat, kmat_v4 * sizeof(uint4)) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_packing_key_create: hipMalloc (key matrix)");
    if (!rc) rc = fill(d_raw, rows, raw_bytes);
    if (!rc) {
        PkMatArgs a{d_raw, k->d_kmat, ctx->p.n, k->n16, k->colgroups};
        rc = launch_kernel(ctx, k_pkmat_build<8, 2>, dim3(4096), dim3(256), 0, ctx->stream, a);
        if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, RTFHE_ERR_HIP, "rtfhe_packing_key_create: k_pkmat_build");
    }
    if (d_raw) (void)hipFree(d_raw);      // the operand form is all the calls read
    return rc ? rc : handle_publish(ctx->pack_keys, std::move(k), out);
}

extern "C" {

int rtfhe_packing_key_create(rtfhe_ctx* ctx, const uint32_t* pk, rtfhe_packing_key** out) {
    return packing_key_create_filled(ctx, pk && out, out, [&](uint32_t* d_raw, size_t, size_t raw_bytes) {
        return hipMemcpy(d_raw, pk, raw_bytes, hipMemcpyHostToDevice) != hipSuccess ? fail(ctx, RTFHE_ERR_HIP, "rtfhe_packing_key_create: hipMemcpy") : 0;
    });
}

// the same key from its seeded form (rtfhe_packing_keygen_seeded): the b halves go up, the masks are made on the device
int rtfhe_packing_key_create_seeded(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* b, rtfhe_packing_key** out) {
    if (ctx && seed && b && out)
        if (int rc = seeded_ready(ctx, "rtfhe_packing_key_create_seeded", RTFHE_SEEDED_UPLOAD, seed, first_row, b, 1, nullptr, (size_t)ctx->p.n * 8 * 3)) return rc;
    return packing_key_create_filled(ctx, seed && b && out, out, [&](uint32_t* d_raw, size_t rows, size_t) {
        if (int rc = stage_seeded(ctx, seed, first_row, b, 1, rows, d_raw)) return rc;
        return hipStreamSynchronize(ctx->stream) != hipSuccess ? fail(ctx, RTFHE_ERR_HIP, "rtfhe_packing_key_create_seeded: k_seeded_expand") : 0;
    });
}

void rtfhe_packing_key_destroy(rtfhe_packing_key* k) {
    handle_destroy(&rtfhe_ctx::pack_keys, k, packing_key_release, [](rtfhe_ctx* ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();      // a pack in flight may still read the matrix
    });
}

int rtfhe_pack_batch_dev(rtfhe_ctx* ctx, const rtfhe_packing_key* pk, const void* d_tlwe, int32_t P, const int32_t* pos, int32_t rep, void* d_out, size_t count,
                         void* stream) {
    std::vector<int32_t> shift;
    if (int rc = pack_ready(ctx, pk, d_tlwe, P, pos, rep, d_out, count, shift)) return rc;
    if (int rc = use(ctx)) return rc;
    if (int rc = device_pointers(ctx, "rtfhe_pack_batch_dev", {d_out, d_tlwe})) return rc;
    return launch_pack(ctx, pk, d_tlwe, P, shift, rep, d_out, count, (hipStream_t)stream);
}

// host buffers: the samples ride in d_a, the result comes back through d_c
int rtfhe_pack_batch(rtfhe_ctx* ctx, const rtfhe_packing_key* pk, const uint32_t* tlwe, int32_t P, const int32_t* pos, int32_t rep, uint32_t* out, size_t count) {
    std::vector<int32_t> shift;
    if (int rc = pack_ready(ctx, pk, tlwe, P, pos, rep, out, count, shift)) return rc;
    const size_t in_bytes = count * (size_t)P * ((size_t)ctx->p.n + 1) * 4, out_bytes = count * 2 * (size_t)ctx->p.N * 4;
    return host_form(ctx, count, {staging_a(ctx), tlwe, in_bytes}, {staging_c(ctx), out, out_bytes, false}, {}, [&](const void* d_tlwe, const StagedIdx*, void* d_out) {
        return launch_pack(ctx, pk, d_tlwe, P, shift, rep, d_out, count, ctx->stream);
    });
}

}  // extern "C"
