// rtfhe_lut.hip -- the tables of programmable bootstrapping (include/rtfhe.h: rtfhe_lut_create[_encrypted], rtfhe_lut_destroy,
// rtfhe_lut_update_dev, rtfhe_lut_accumulate_dev, rtfhe_lut_read_dev): a copy of the rows on every entry of the context, its release, and the
// three stream-ordered row calls of an encrypted table -- rewrite (e.g. from a packing key switch), wrapping sum (k_trlwe_accumulate, e.g. of a
// demultiplexer's leaves), read.  The calls that bootstrap with a table are in rtfhe_batch.hip.
#include "rtfhe_host.hpp"

#include "rtfhe_kernels_lut.hpp"

using namespace rtfhe;
using namespace rtfhe_host;

namespace {

// lut_upload's fill for rows the caller holds in full
auto copy_rows(const uint32_t* tv) {
    return [tv](rtfhe_ctx* c, void* p, size_t bytes) {
        return hipMemcpy(p, tv, bytes, hipMemcpyHostToDevice) != hipSuccess ? fail(c, RTFHE_ERR_HIP, "rtfhe_lut_create: hipMemcpy") : 0;
    };
}

// the rows of a table (plain: [n_lut][N] test polynomials; encrypted: [n_lut][2][N] TRLWEs) uploaded to every entry of the context
// (fill(c, p, bytes) brings the rows into p on entry c, done when it returns: the caller's copy, or a seeded table's expansion)
template <typename Fill>
int lut_upload(rtfhe_ctx* ctx, int32_t n_lut, bool encrypted, rtfhe_lut** out, Fill fill) {
    *out = nullptr;
    const size_t bytes = (size_t)n_lut * ctx->p.N * (encrypted ? 2 : 1) * 4;
    NewHandle<rtfhe_lut> lut = new_handle(ctx, lut_release);      // (lut_release frees as many copies as d_tv lists)
    lut->n_lut = n_lut;
    lut->encrypted = encrypted;
    const int entries = 1 + (int)ctx->peers.size();
    int rc = 0;
    for (int d = 0; d < entries && !rc; d++) {
        rtfhe_ctx* c = d ? ctx->peers[d - 1] : ctx;
        void* p = nullptr;
        rc = use(c);
        if (!rc && hipMalloc(&p, bytes) != hipSuccess) rc = fail(c, RTFHE_ERR_HIP, "rtfhe_lut_create: hipMalloc");
        if (p) lut->d_tv.push_back((uint32_t*)p);
        if (!rc) rc = fill(c, p, bytes);
        if (rc && c != ctx) rc = fail(ctx, rc, "device " + std::to_string(c->device) + ": " + c->err);
    }
    (void)hipSetDevice(ctx->device);
    return rc ? rc : handle_publish(ctx->luts, std::move(lut), out);
}

// What the three row calls check before anything is queued, in this order: the handle, the caller's pointer, an encrypted table, a
// single-device context, the row range, the pointer's memory.  name: the call's; does: the verb phrase of its "this one is plain" message.
// out: the table's context, made current.
int rows_ready(const rtfhe_lut* lut, const void* d_ptr, int32_t first, int32_t n, const char* name, const char* does, rtfhe_ctx*& ctx) {
    ctx = lut ? lut->ctx : nullptr;
    if (int rc = handles_ready(ctx, {ref(lut)})) return rc;
    if (!d_ptr) return fail(ctx, RTFHE_ERR_INVALID, "null argument");
    if (!lut->encrypted)
        return fail(ctx, RTFHE_ERR_INVALID, std::string(name) + " " + does + " the rows of an encrypted table (rtfhe_lut_create_encrypted); this one is plain");
    if (!ctx->peers.empty()) return fail(ctx, RTFHE_ERR_INVALID, std::string(name) + ": a multi-device context holds one copy of the table per device; not supported");
    if (first < 0 || n < 0 || (long long)first + n > lut->n_lut)
        return fail(ctx, RTFHE_ERR_INVALID, "rows [" + std::to_string(first) + ", " + std::to_string((long long)first + n) + ") are outside the table's [0, " +
                                            std::to_string(lut->n_lut) + ")");
    if (int rc = use(ctx)) return rc;
    return device_pointers(ctx, name, {d_ptr});
}

}  // namespace

namespace rtfhe_host {

void lut_release(rtfhe_lut* lut) {
    rtfhe_ctx* ctx = lut->ctx;
    for (size_t d = 0; d < lut->d_tv.size(); d++) {
        (void)hipSetDevice(d ? ctx->peers[d - 1]->device : ctx->device);
        (void)hipFree(lut->d_tv[d]);
    }
    lut->d_tv.clear();
    (void)hipSetDevice(ctx->device);
}

}  // namespace rtfhe_host

extern "C" {

int rtfhe_lut_create(rtfhe_ctx* ctx, const uint32_t* tv, int32_t n_lut, rtfhe_lut** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!tv || !out || n_lut < 1) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_lut_create: null argument or n_lut < 1");
    return lut_upload(ctx, n_lut, false, out, copy_rows(tv));
}

int rtfhe_lut_create_encrypted(rtfhe_ctx* ctx, const uint32_t* trlwe, int32_t n_lut, rtfhe_lut** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!trlwe || !out || n_lut < 1) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_lut_create_encrypted: null argument or n_lut < 1");
    return lut_upload(ctx, n_lut, true, out, copy_rows(trlwe));
}

// the same table from its seeded form: on every entry the b halves go up and the masks are made there
int rtfhe_lut_create_encrypted_seeded(rtfhe_ctx* ctx, const uint32_t* seed, uint64_t first_row, const uint32_t* b, int32_t n_lut, rtfhe_lut** out) {
    if (!ctx) return fail(nullptr, RTFHE_ERR_INVALID, "null context");
    if (!seed || !b || !out || n_lut < 1) return fail(ctx, RTFHE_ERR_INVALID, "rtfhe_lut_create_encrypted_seeded: null argument or n_lut < 1");
    if (int rc = seeded_ready(ctx, "rtfhe_lut_create_encrypted_seeded", RTFHE_SEEDED_UPLOAD, seed, first_row, b, 1, nullptr, (size_t)n_lut)) return rc;
    return lut_upload(ctx, n_lut, true, out, [&](rtfhe_ctx* c, void* p, size_t) {
        if (int rc = stage_seeded(c, seed, first_row, b, 1, (size_t)n_lut, p)) return rc;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(c, RTFHE_ERR_HIP, "rtfhe_lut_create_encrypted_seeded: k_seeded_expand");
        return 0;
    });
}

void rtfhe_lut_destroy(rtfhe_lut* lut) { handle_destroy(&rtfhe_ctx::luts, lut, lut_release); }

int rtfhe_lut_update_dev(rtfhe_lut* lut, const void* d_trlwe, int32_t first, int32_t n, void* stream) {
    rtfhe_ctx* ctx = nullptr;
    if (int rc = rows_ready(lut, d_trlwe, first, n, "rtfhe_lut_update_dev", "rewrites", ctx)) return rc;
    if (n == 0) return 0;
    const size_t row = 2 * (size_t)ctx->p.N;
    HIPCHECK(ctx, hipMemcpyAsync(lut->d_tv[0] + (size_t)first * row, d_trlwe, (size_t)n * row * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int rtfhe_lut_accumulate_dev(rtfhe_lut* lut, const void* d_trlwe, int32_t first, int32_t n, size_t count, void* stream) {
    rtfhe_ctx* ctx = nullptr;
    if (int rc = rows_ready(lut, d_trlwe, first, n, "rtfhe_lut_accumulate_dev", "adds into", ctx)) return rc;
    if (count < 1 || count > (size_t)0x7fffffff) return fail(ctx, RTFHE_ERR_INVALID, "count = " + std::to_string(count) + " is outside [1, 2^31)");
    if (n == 0) return 0;
    const size_t row = 2 * (size_t)ctx->p.N;
    TrlweAccumulateArgs a{lut->d_tv[0] + (size_t)first * row, (const uint32_t*)d_trlwe, (size_t)n * row, (int32_t)count};
    return launch_kernel(ctx, k_trlwe_accumulate, dim3((unsigned)((a.words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
}

int rtfhe_lut_read_dev(const rtfhe_lut* lut, void* d_out, int32_t first, int32_t n, void* stream) {
    rtfhe_ctx* ctx = nullptr;
    if (int rc = rows_ready(lut, d_out, first, n, "rtfhe_lut_read_dev", "copies", ctx)) return rc;
    if (n == 0) return 0;
    const size_t row = 2 * (size_t)ctx->p.N;
    HIPCHECK(ctx, hipMemcpyAsync(d_out, lut->d_tv[0] + (size_t)first * row, (size_t)n * row * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

}  // extern "C"
