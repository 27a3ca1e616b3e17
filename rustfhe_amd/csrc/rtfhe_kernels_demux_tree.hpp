// rtfhe_kernels_demux_tree.hpp -- CMUX demultiplexer tree: one TRLWE into leaf `addr` of 2^d, the address given as TRGSW-encrypted bits
// (include/rtfhe.h: rtfhe_demux_tree_batch).  The wrapping sum of such leaves into the rows of an encrypted table (rtfhe_lut_accumulate_dev)
// is the table unit's: rtfhe_kernels_lut.hpp.
//
// The tree of rtfhe_kernels_cmux_tree.hpp run backwards.  One launch per level over the nodes of that level of every lookup; a wave owns one
// INPUT node and writes its two children:
//   child[2j+1] = cross(S_k, node_j)             (TRGSWRepF::cross, hom_nand/src/trgsw.rs:264-306)
//   child[2j]   = node_j - child[2j+1]           wrapping on every word
// Level t has 2^t nodes per lookup and uses selector k = demux_level_selector(depth, t) = depth - 1 - t: the most significant address bit
// splits first, so that after the last level leaf i sits at row i.  Level 0 reads x, every other level the previous level's buffer; the last
// level writes out.  The product is cmux_step<.., CMUX = false> itself (rtfhe_kernels.hpp), called, not restated; ROUNDED is cmux_step's.
// k_cmux_tree's launch shape and LDS carve.  Instantiated in rtfhe_cmux_tree.hip.
#pragma once

#include "rtfhe_kernels_cmux_tree.hpp"

namespace rtfhe {

constexpr int DEMUX_TREE_MAX_DEPTH = CMUX_TREE_MAX_DEPTH;

// the selector (address bit) that demux level `level` of a depth-`depth` tree splits on
__host__ __device__ constexpr int demux_level_selector(int depth, int level) { return depth - 1 - level; }

struct DemuxTreeArgs {
    const cplx* tw;
    const cplx* sel;           // selector spectra, device layout [n_sel][2l][2][R][64]
    const int32_t* sel_idx;    // [count][depth], entry k = address bit k; null: lookup g uses g * depth + k
    const uint32_t* src;       // this level's input nodes [count << level][2][N]: x at level 0, else the previous level's buffer
    uint32_t* dst;             // this level's children [count << (level + 1)][2][N]; the last level: out [count][2^depth][2][N]
    int32_t* fault;            // set to 1 when a lookup was skipped for an out-of-range index
    int32_t count, depth, level;
    int32_t n_sel;
};

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_demux_tree(const DemuxTreeArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    static_assert(cmux_tree_lds_bytes<LOGN, WAVES>() <= (size_t)160 * 1024, "k_demux_tree: the LDS carve of this (N, waves) shape passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = leveled_stage_twiddles<LOGN, WAVES>(smem, a.tw, tid);

    const long long q = (long long)blockIdx.x * WAVES + wave;      // input node number within the level: lookup g, node j = q - (g << level)
    if (q >= ((long long)a.count << a.level)) return;
    const int g = (int)(q >> a.level);

    // every index of lookup g is checked at every level (a handful of wave-uniform loads): a bad lookup is skipped whole
    bool ok = true;
    int s = 0;
    const int kl = demux_level_selector(a.depth, a.level);
    for (int k = 0; k < a.depth; k++) {
        const int sk = a.sel_idx ? a.sel_idx[(size_t)g * a.depth + k] : g * a.depth + k;
        ok = ok && (unsigned)sk < (unsigned)a.n_sel;
        if (k == kl) s = sk;
    }
    if (!ok) { if (a.fault) *a.fault = 1; return; }

    const WaveLds w = leveled_wave_lds<LOGN, WAVES>(smem, wave);
    double* xbuf = w.xbuf;
    uint32_t* accbuf = w.accbuf;

    const uint32_t* node = a.src + (size_t)q * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) accbuf[c] = node[c];
    wave_lds_sync();
    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
    cmux_step<LOGN, L, BGBIT, false, DUAL, ROUNDED>(accbuf, 0, a.sel + (size_t)s * trgsw_cplx, TwStage<LOGN>::fwd(tw), TwStage<LOGN>::inv_small(tw),
                                                    TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);

    // children 2j and 2j+1 of lookup g are rows 2q and 2q+1 of the level's output (g << (level + 1)) + 2j = 2q.  The node is read a second
    // time for the difference, cmux_select's trade: the L2 still holds its 2N words
    uint32_t* lo = a.dst + (size_t)(2 * q) * 2 * N;
    uint32_t* hi = lo + 2 * N;
    for (int c = lane; c < 2 * N; c += 64) {
        const uint32_t p = accbuf[c];
        hi[c] = p;
        lo[c] = node[c] - p;
    }
}

}  // namespace rtfhe
