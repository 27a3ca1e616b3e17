// rtfhe_kernels_trgsw_rotate.hpp -- TRGSW blind rotation: a TRLWE rotated by encrypted address bits (include/rtfhe.h: rtfhe_trgsw_rotate_batch).
//
// One launch, a wave owns one lookup and runs all of its steps on the wave-private accumulator in LDS:
//   acc <- cmux(S_k, X^{rot[k]} * acc, acc) = cross(S_k, X^{rot[k]} * acc - acc) + acc        (one step of TFHE::blind_rotate, tfhe.rs:103-110,
//                                                                                              the key entry replaced by selector S_k, abar_i by rot[k])
// then stores the 2N words -- or, in the extract form, sample extract index 0 (trlwe.rs:110-121) in the batch key switch's operand order
// (ext_slot).  The step is cmux_step<.., CMUX = true> itself (rtfhe_kernels.hpp), called, not restated: the kernels that existed before
// compile to what they did.  ROUNDED is cmux_step's, as in k_cmux_tree.  Instantiated in rtfhe_cmux_tree.hip.
//
// A lookup with a selector index outside the set is skipped whole and its output row stays as it was.  In the extract form the batch key
// switch that follows writes every row: the skipped lookup's wave parks the row in its own sample slots and k_rows_restore, launched behind the
// key switch, puts it back -- the one parked-row rule of rtfhe_kernels.hpp (park_row, whose loop this kernel has to restate: see there), with
// (sel_idx, depth, n_sel) as the restore's index rule.
#pragma once

#include "rtfhe_kernels_cmux_tree.hpp"

namespace rtfhe {

constexpr int TRGSW_ROTATE_MAX_DEPTH = CMUX_TREE_MAX_DEPTH;

struct TrgswRotateArgs {
    const cplx* tw;
    const cplx* sel;           // selector spectra, device layout [n_sel][2l][2][R][64]
    const int32_t* sel_idx;    // [count][depth], entry k = the selector of step k; null: lookup g uses g * depth + k
    const uint32_t* in;        // [count][2][N] (b then a); may be exactly `out`
    uint32_t* out;             // [count][2][N] (unused in the extract form)
    uint32_t* ext;             // extract form: lvl1 samples in the batch key switch's operand order
    uint32_t* ks_out;          // extract form: the key switch's output [count][n+1], whose rows of skipped lookups are put back (k_rows_restore)
    int32_t* fault;            // set to 1 when a lookup was skipped for an out-of-range index
    int32_t count, depth;
    int32_t n_sel, n;
    int32_t rot[TRGSW_ROTATE_MAX_DEPTH];      // the exponents in [0, 2N), copied from the caller's host array when the launch is enqueued
};

// are all selector indices of lookup g inside the set?  (wave-uniform)
__device__ __forceinline__ bool trgsw_rotate_ok(const TrgswRotateArgs& a, long long g) {
    bool ok = true;
    for (int k = 0; k < a.depth; k++) {
        const int sk = a.sel_idx ? a.sel_idx[(size_t)g * a.depth + k] : (int)g * a.depth + k;
        ok = ok && (unsigned)sk < (unsigned)a.n_sel;
    }
    return ok;
}

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_trgsw_rotate(const TrgswRotateArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    static_assert(cmux_tree_lds_bytes<LOGN, WAVES>() <= (size_t)160 * 1024, "k_trgsw_rotate: the LDS carve of this (N, waves) shape passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = leveled_stage_twiddles<LOGN, WAVES>(smem, a.tw, tid);

    const long long g = (long long)blockIdx.x * WAVES + wave;
    if (g >= a.count) return;

    // every index of the lookup is checked before its row is touched (a handful of wave-uniform loads): a bad lookup is skipped whole
    if (!trgsw_rotate_ok(a, g)) {
        if (a.fault) *a.fault = 1;
        if (a.ext) {
            // park_row (rtfhe_kernels.hpp) restated: through the helper all four kernels come out with other code (scripts/isa/snapshot.py)
            const uint32_t* keep = a.ks_out + (size_t)g * (a.n + 1);
            for (int c = lane; c <= a.n; c += 64) *ext_slot(a.ext, (int)g, c, N) = keep[c];
        }
        return;
    }

    // leveled_wave_lds restated: through the helper the N = 2048 kernel comes out with other spill code (scripts/isa/snapshot.py)
    unsigned char* wbase = smem + (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)wave * bootstrap_wave_lds_bytes<LOGN>(0, DUAL);
    double* xbuf = reinterpret_cast<double*>(wbase);
    uint32_t* accbuf = reinterpret_cast<uint32_t*>(wbase + (size_t)G::XSLOTS * sizeof(double) * (DUAL ? 2 : 1));

    // the whole row goes into LDS before anything is stored: out may be the input buffer
    const uint32_t* row = a.in + (size_t)g * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) accbuf[c] = row[c];
    wave_lds_sync();

    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
#pragma unroll 1
    for (int k = 0; k < a.depth; k++) {
        const int sk = __builtin_amdgcn_readfirstlane(a.sel_idx ? a.sel_idx[(size_t)g * a.depth + k] : (int)g * a.depth + k);
        const int r = a.rot[k];
        cmux_step<LOGN, L, BGBIT, true, DUAL, ROUNDED>(accbuf, r, a.sel + (size_t)sk * trgsw_cplx, TwStage<LOGN>::fwd(tw), TwStage<LOGN>::inv_small(tw),
                                              TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);
    }

    if (a.ext) {
        // sample extract index 0 (trlwe.rs:110-121): a'_0 = a_0, a'_c = -a_{N - c} above; b' = b_0
        for (int c = lane; c < N; c += 64) *ext_slot(a.ext, (int)g, c, N) = c == 0 ? accbuf[N] : 0u - accbuf[2 * N - c];
        if (lane == 0) *ext_slot(a.ext, (int)g, N, N) = accbuf[0];
        return;
    }
    uint32_t* o = a.out + (size_t)g * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) o[c] = accbuf[c];
}

}  // namespace rtfhe
