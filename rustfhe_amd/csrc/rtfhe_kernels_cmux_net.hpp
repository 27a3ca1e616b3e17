// rtfhe_kernels_cmux_net.hpp -- CMUX netlists: decision diagrams over TRGSW-encrypted inputs (include/rtfhe.h: rtfhe_cmux_circuit_create).
//
// Every node of every replica owns a slot of the node buffer [count][n_nodes][2][N].  One launch of k_cmux_net per level of the levelised
// netlist, a wave owns one (replica, node of the level):
//   value_i = cmux(S, X^rot * value(hi), value(lo)) = cross(S, X^rot * hi - lo) + lo          (TRGSWRepF::cmux, hom_nand/src/trgsw.rs:319-321;
//                                                                                              X^rot: rotated_coef, utils/src/math.rs:85-132)
// hi and lo are slots of lower levels or table rows (a plain row tv is the trivial TRLWE (tv, 0)).  The product is
// cmux_step<.., CMUX = false> itself (rtfhe_kernels.hpp), called, not restated, on the tree's launch shape and LDS carve; ROUNDED is
// cmux_step's, as in k_cmux_tree.
// k_cmux_net_check runs first (a wave per replica: its device-resident indices), k_cmux_net_out last (a wave per (replica, output): the
// node copied to d_out, or its sample extract in the batch key switch's operand order).  Instantiated in rtfhe_cmux_net.hip.
#pragma once

#include "rtfhe_kernels_cmux_tree.hpp"

namespace rtfhe {

struct CmuxNetArgs {
    const cplx* tw;
    const cplx* sel;           // selector spectra, device layout [n_sel][2l][2][R][64]
    const int32_t* sel_idx;    // [count][n_vars]; null: replica g uses g * n_vars + v
    const int32_t* row0;       // [count] the table row leaf 0 of replica g names; null: 0
    const uint32_t* table;     // plain: [n_lut][N]; encrypted: [n_lut][2][N] (b then a)
    uint32_t* nodes;           // [count][n_nodes][2][N]
    int32_t* ok;               // [count] 1: the replica's indices are inside their ranges (written by k_cmux_net_check)
    const int32_t* var;        // [n_nodes] the description, on the device
    const int32_t* hi;
    const int32_t* lo;
    const int32_t* rot;
    const int32_t* level;      // k_cmux_net: the n_level node numbers of this launch's level
    const int32_t* out_ref;    // k_cmux_net_out: [n_out]
    const int32_t* out_coef;   // ... [n_out], extract form; null: TRLWE form
    uint32_t* out;             // ... TRLWE form: [count][n_out][2][N]
    uint32_t* ext;             // ... extract form: lvl1 samples g * n_out + o in the batch key switch's operand order
    int32_t* fault;            // set to 1 when a replica was skipped for an out-of-range index
    int32_t count, n_nodes, n_vars, n_level, n_out;
    int32_t n_sel, n_lut;
    int32_t leaf_min, leaf_max;      // the smallest and the largest leaf the netlist names
    int32_t enc;               // the table holds TRLWE rows
};

// acc <- cmux(S, X^r * hi, lo) on the wave-private accumulator, beside cmux_select (rtfhe_kernels_cmux_tree.hpp): the rotated read of hi
// comes from global memory, and either child may be a plain table row, whose a-half (null) reads as zero.
template <int LOGN, int L, int BGBIT, bool DUAL, bool ROUNDED>
__device__ __forceinline__ void cmux_select_rotated(uint32_t* __restrict__ accbuf, const cplx* __restrict__ S, int r, const uint32_t* __restrict__ b1,
                                                    const uint32_t* __restrict__ a1, const uint32_t* __restrict__ b0, const uint32_t* __restrict__ a0,
                                                    const cplx* __restrict__ twf, const cplx* __restrict__ twi, const cplx* __restrict__ twi_big,
                                                    double* __restrict__ xbuf, int lane) {
    constexpr int N = 1 << LOGN;
    for (int c = lane; c < N; c += 64) {
        accbuf[c] = rotated_coef<LOGN>(b1, c, r) - b0[c];
        accbuf[N + c] = (a1 ? rotated_coef<LOGN>(a1, c, r) : 0u) - (a0 ? a0[c] : 0u);
    }
    wave_lds_sync();
    cmux_step<LOGN, L, BGBIT, false, DUAL, ROUNDED>(accbuf, 0, S, twf, twi, twi_big, xbuf, lane);
    for (int c = lane; c < N; c += 64) {
        accbuf[c] += b0[c];
        if (a0) accbuf[N + c] += a0[c];
    }
    wave_lds_sync();
}

// a wave per replica: all n_vars selector indices against the set, row0 against the leaves the netlist names.  Nothing is read through them.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_cmux_net_check(const CmuxNetArgs a) {
    const int lane = threadIdx.x & 63;
    const long long g = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (g >= a.count) return;
    bool good = true;
    if (a.sel_idx)
        for (int v = lane; v < a.n_vars; v += 64) good = good && (unsigned)a.sel_idx[(size_t)g * a.n_vars + v] < (unsigned)a.n_sel;
    if (a.row0) {
        const long long r0 = a.row0[g];
        good = good && r0 + a.leaf_min >= 0 && r0 + a.leaf_max < (long long)a.n_lut;
    }
    const bool all = __all(good);
    if (lane == 0) {
        a.ok[g] = all ? 1 : 0;
        if (!all && a.fault) *a.fault = 1;
    }
}

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_cmux_net(const CmuxNetArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    constexpr bool DUAL = bootstrap_dual_xbuf(LOGN, WAVES);
    static_assert(cmux_tree_lds_bytes<LOGN, WAVES>() <= (size_t)160 * 1024, "k_cmux_net: the LDS carve of this (N, waves) shape passes the 160 KiB of a CU");
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = leveled_stage_twiddles<LOGN, WAVES>(smem, a.tw, tid);

    const long long q = (long long)blockIdx.x * WAVES + wave;      // replica g, node j of the level
    if (q >= (long long)a.count * a.n_level) return;
    const int g = (int)(q / a.n_level), j = (int)(q % a.n_level);
    if (!a.ok[g]) return;                                           // a replica with a bad index is skipped whole
    const int i = __builtin_amdgcn_readfirstlane(a.level[j]);
    const int s = __builtin_amdgcn_readfirstlane(a.sel_idx ? a.sel_idx[(size_t)g * a.n_vars + a.var[i]] : g * a.n_vars + a.var[i]);
    const int r = a.rot ? a.rot[i] : 0;
    const long long r0 = a.row0 ? a.row0[g] : 0;

    const WaveLds w = leveled_wave_lds<LOGN, WAVES>(smem, wave);
    double* xbuf = w.xbuf;
    uint32_t* accbuf = w.accbuf;

    uint32_t* slots = a.nodes + (size_t)g * a.n_nodes * 2 * N;
    const size_t roww = a.enc ? (size_t)2 * N : (size_t)N;
    const uint32_t *bb[2], *aa[2];                                  // 0: lo, 1: hi
    const int ref[2] = {a.lo[i], a.hi[i]};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (ref[k] >= 0) {
            bb[k] = slots + (size_t)ref[k] * 2 * N;
            aa[k] = bb[k] + N;
        } else {
            bb[k] = a.table + (size_t)(r0 + (-1ll - ref[k])) * roww;
            aa[k] = a.enc ? bb[k] + N : nullptr;
        }
    }
    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
    cmux_select_rotated<LOGN, L, BGBIT, DUAL, ROUNDED>(accbuf, a.sel + (size_t)s * trgsw_cplx, r, bb[1], aa[1], bb[0], aa[0], TwStage<LOGN>::fwd(tw),
                                              TwStage<LOGN>::inv_small(tw), TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);
    uint32_t* o = slots + (size_t)i * 2 * N;
    for (int c = lane; c < 2 * N; c += 64) o[c] = accbuf[c];
}

// a wave per (replica, output).  A skipped replica's TRLWE rows keep their bytes; in the extract form its samples are zeroed, so that the key
// switch behind (which writes every row) gives all-zero rows and never reads stale words.
template <int LOGN, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_cmux_net_out(const CmuxNetArgs a) {
    constexpr int N = 1 << LOGN;
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= (long long)a.count * a.n_out) return;
    const int g = (int)(q / a.n_out), o = (int)(q % a.n_out);
    const bool good = a.ok[g] != 0;
    if (!a.out_coef) {
        if (!good) return;
        const uint32_t* src = a.nodes + ((size_t)g * a.n_nodes + a.out_ref[o]) * 2 * N;
        uint32_t* dst = a.out + (size_t)q * 2 * N;
        for (int c = lane; c < 2 * N; c += 64) dst[c] = src[c];
        return;
    }
    if (!good) {
        for (int c = lane; c <= N; c += 64) *ext_slot(a.ext, (int)q, c, N) = 0u;
        return;
    }
    // sample extract index cf (trlwe.rs:110-121): a'_c = a_{cf - c} for c <= cf, -a_{N + cf - c} above; b' = b_cf
    const uint32_t* src = a.nodes + ((size_t)g * a.n_nodes + a.out_ref[o]) * 2 * N;
    const int cf = a.out_coef[o];
    for (int c = lane; c < N; c += 64) *ext_slot(a.ext, (int)q, c, N) = c <= cf ? src[N + cf - c] : 0u - src[2 * N + cf - c];
    if (lane == 0) *ext_slot(a.ext, (int)q, N, N) = src[cf];
}

}  // namespace rtfhe
