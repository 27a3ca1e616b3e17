// rtfhe_kernels_cmux_tree.hpp -- CMUX-tree table lookup with caller-supplied TRGSW selectors (include/rtfhe.h: rtfhe_cmux_tree_batch).
//
// One launch per tree level over the nodes of that level of every lookup; a wave owns one node:
//   r' = cmux(S_k, r_{2j+1}, r_{2j}) = cross(S_k, r_{2j+1} - r_{2j}) + r_{2j}      (TRGSWRepF::cmux, hom_nand/src/trgsw.rs:319-321)
// Level 0 reads its two children from the table (a plain row tv is the trivial TRLWE (tv, 0)), every other level from the previous level's
// buffer; the last level writes the lookup's result -- or, in the extract form, sample extract index coef[g] of it (trlwe.rs:110-121) in the
// batch key switch's operand order (ext_slot).  The product is cmux_step<.., CMUX = false> itself (rtfhe_kernels.hpp), called, not restated:
// the kernels that existed before compile to what they did.  ROUNDED is cmux_step's: the rounded gadget decomposition of the leveled mode
// (include/rtfhe.h: rtfhe_set_leveled_decomposition), two other constants and nothing else.  Instantiated in rtfhe_cmux_tree.hip.
#pragma once

#include "rtfhe_kernels.hpp"

namespace rtfhe {

constexpr int CMUX_TREE_MAX_DEPTH = 16;

struct CmuxTreeArgs {
    const cplx* tw;
    const cplx* sel;           // selector spectra, device layout [n_sel][2l][2][R][64]
    const int32_t* sel_idx;    // [count][depth], entry k = the selector of level k (address bit k); null: lookup g uses g * depth + k
    const int32_t* row0;       // [count] first table row of lookup g; null: 0
    const int32_t* coef;       // extract form: [count] the coefficient to extract; null: 0
    const uint32_t* table;     // plain: [n_lut][N]; encrypted: [n_lut][2][N] (b then a)
    const uint32_t* src;       // level > 0: the previous level's nodes [count << (depth - level)][2][N]
    uint32_t* dst;             // this level's nodes [count << (depth - 1 - level)][2][N]; the last level: out [count][2][N] (unused in the extract form)
    uint32_t* ext;             // extract form, last level: lvl1 samples in the batch key switch's operand order
    int32_t* fault;            // set to 1 when a lookup was skipped for an out-of-range index
    int32_t count, depth, level;
    int32_t n_sel, n_lut;
    int32_t enc;               // the table holds TRLWE rows
};

// per-wave LDS of k_cmux_tree: the exchange buffer(s) of the transforms, then the accumulator (b then a)
template <int LOGN, int WAVES>
__host__ __device__ constexpr size_t cmux_tree_lds_bytes() { return bootstrap_lds_bytes<LOGN>(WAVES, 0, bootstrap_dual_xbuf(LOGN, WAVES)); }

// ---- the frame the four leveled kernels (k_cmux_tree, k_demux_tree, k_trgsw_rotate, k_cmux_net) open with ----
// In two halves, because the kernels leave early in between.  First the twiddles of the workgroup into the head of
// its LDS and the one barrier; from there on waves never synchronise with each other.
template <int LOGN, int WAVES>
__device__ __forceinline__ cplx* leveled_stage_twiddles(unsigned char* smem, const cplx* tw_global, int tid) {
    cplx* tw = reinterpret_cast<cplx*>(smem);
    TwStage<LOGN>::stage(tw, tw_global, tid, 64 * WAVES);
    __syncthreads();
    return tw;
}
// ... then the wave's own carve behind them: the exchange buffer(s) of the transforms, then the accumulator (b then a)
struct WaveLds { double* xbuf; uint32_t* accbuf; };
template <int LOGN, int WAVES>
__device__ __forceinline__ WaveLds leveled_wave_lds(unsigned char* smem, int wave) {
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    unsigned char* wbase = smem + (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)wave * bootstrap_wave_lds_bytes<LOGN>(0, DUAL);
    return {reinterpret_cast<double*>(wbase), reinterpret_cast<uint32_t*>(wbase + (size_t)Geo<LOGN>::XSLOTS * sizeof(double) * (DUAL ? 2 : 1))};
}

// acc <- cmux(S, r1, r0) on the wave-private accumulator: the difference into LDS, the external product in place, r0 added back from where it
// came (a second read of 2N words that the L2 still holds costs less than 2N / 64 registers live across the product).  A null a-half (plain
// table rows) reads as zero.
template <int LOGN, int L, int BGBIT, bool DUAL, bool ROUNDED>
__device__ __forceinline__ void cmux_select(uint32_t* __restrict__ accbuf, const cplx* __restrict__ S, const uint32_t* __restrict__ b1,
                                            const uint32_t* __restrict__ a1, const uint32_t* __restrict__ b0, const uint32_t* __restrict__ a0,
                                            const cplx* __restrict__ twf, const cplx* __restrict__ twi, const cplx* __restrict__ twi_big,
                                            double* __restrict__ xbuf, int lane) {
    constexpr int N = 1 << LOGN;
    for (int c = lane; c < N; c += 64) {
        accbuf[c] = b1[c] - b0[c];
        accbuf[N + c] = a1 ? a1[c] - a0[c] : 0u;
    }
    wave_lds_sync();
    cmux_step<LOGN, L, BGBIT, false, DUAL, ROUNDED>(accbuf, 0, S, twf, twi, twi_big, xbuf, lane);
    for (int c = lane; c < N; c += 64) {
        accbuf[c] += b0[c];
        if (a0) accbuf[N + c] += a0[c];
    }
    wave_lds_sync();
}

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_cmux_tree(const CmuxTreeArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    static_assert(cmux_tree_lds_bytes<LOGN, WAVES>() <= (size_t)160 * 1024, "k_cmux_tree: the LDS carve of this (N, waves) shape passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = leveled_stage_twiddles<LOGN, WAVES>(smem, a.tw, tid);

    const int lvl_bits = a.depth - 1 - a.level;            // log2 of this level's nodes per lookup
    const long long q = (long long)blockIdx.x * WAVES + wave;      // node number within the level: lookup g, node j
    if (q >= ((long long)a.count << lvl_bits)) return;
    const int g = (int)(q >> lvl_bits), j = (int)(q & ((1ll << lvl_bits) - 1));

    // every index of lookup g is checked at every level (a handful of wave-uniform loads): a bad lookup is skipped whole
    const int r0 = a.row0 ? a.row0[g] : 0;
    const int cf = a.coef ? a.coef[g] : 0;
    bool ok = r0 >= 0 && (long long)r0 + (1ll << a.depth) <= (long long)a.n_lut && (unsigned)cf < (unsigned)N;
    int s = 0;
    for (int k = 0; k < a.depth; k++) {
        const int sk = a.sel_idx ? a.sel_idx[(size_t)g * a.depth + k] : g * a.depth + k;
        ok = ok && (unsigned)sk < (unsigned)a.n_sel;
        if (k == a.level) s = sk;
    }
    if (!ok) { if (a.fault) *a.fault = 1; return; }

    const WaveLds w = leveled_wave_lds<LOGN, WAVES>(smem, wave);
    double* xbuf = w.xbuf;
    uint32_t* accbuf = w.accbuf;

    const uint32_t *b0, *a0, *b1, *a1;
    if (a.level == 0) {
        const size_t roww = a.enc ? (size_t)2 * N : (size_t)N;
        const uint32_t* p0 = a.table + ((size_t)r0 + 2 * (size_t)j) * roww;
        b0 = p0; b1 = p0 + roww;
        a0 = a.enc ? b0 + N : nullptr; a1 = a.enc ? b1 + N : nullptr;
    } else {
        const uint32_t* p0 = a.src + (size_t)(2 * q) * 2 * N;
        b0 = p0; a0 = p0 + N; b1 = p0 + 2 * N; a1 = p0 + 3 * N;
    }
    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
    cmux_select<LOGN, L, BGBIT, DUAL, ROUNDED>(accbuf, a.sel + (size_t)s * trgsw_cplx, b1, a1, b0, a0, TwStage<LOGN>::fwd(tw), TwStage<LOGN>::inv_small(tw),
                                      TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);

    if (a.ext && lvl_bits == 0) {
        // sample extract index cf (trlwe.rs:110-121): a'_c = a_{cf - c} for c <= cf, -a_{N + cf - c} above; b' = b_cf
        for (int c = lane; c < N; c += 64) *ext_slot(a.ext, g, c, N) = c <= cf ? accbuf[N + cf - c] : 0u - accbuf[2 * N + cf - c];
        if (lane == 0) *ext_slot(a.ext, g, N, N) = accbuf[cf];
        return;
    }
    uint32_t* o = a.dst + (size_t)q * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) o[c] = accbuf[c];
}

}  // namespace rtfhe
