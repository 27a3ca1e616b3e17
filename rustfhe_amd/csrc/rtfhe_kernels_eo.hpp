// rtfhe_kernels_eo.hpp -- N = 2048 (BASELINE config 5): two waves per transform, split by the PARITY of the point index.
//
// At N = 2048 a polynomial's transform has 1024 complex points: 16 per lane in one wavefront, which with three digit rows side by side does not
// fit the register file (k_bootstrap<11>, one wave per gate, lives in 512 registers with ~790 AGPR shuffles per step at the lone-wave issue rate).
// So the two waves of a gate share every transform.  Wave H owns the points of parity H: i = 2 j + H, j in [0, 512).  Every radix-2 stage of the
// reference network pairs i with i + halfnn (forward, decimation in frequency, spqlios-fft-impl.cpp:526-572; inverse, decimation in time,
// :315-363), and for halfnn >= 2 both have the same parity: NINE of the ten stages stay inside a wave -- twist, halfnn = 512 ... 4 (eight
// twiddled stages), and this parity's half of the size-4 stage (:575-603 / :289-310) -- as a 512-point network in j of exactly the shape the
// N = 1024 kernels run (8 points per lane, three in-register passes of three stages, two wave-private exchanges), with the twiddle of pair
// (i, i + halfnn) = entry (i mod halfnn) = 2 (j mod halfnn/2) + H of the reference's stage table.  Only the size-2 stage (halfnn = 1: x0 + x1,
// x0 + (-x1), no twiddle, :606-634 / :248-269) crosses the waves: it is the LAST stage of the forward transform and the FIRST of the inverse.
//   * both waves execute the same instruction stream (wave 1's only differences: table pointers, and "partner + (-mine)" where wave 0 has
//     "mine + partner") -- the work is balanced by construction;
//   * the forward trade comes after a row's pass 3: the NEXT row's pass 3 (and, for the last row, the first multiply-accumulates) run between
//     a row's arrival flag and the wait for the partner's -- no wave sits at a synchronisation with nothing to issue;
//   * gather, decomposition and twist are wave-private: no first-stage trade at all;
//   * the stage across the waves sits right next to the pointwise multiply-accumulate, whose layout is free: each wave finishes BOTH outputs of the
//     butterflies of half of the indices k (it sends 4 of its 8 values per lane and receives 4: half-width trade), and the key is stored in that
//     layout (k_bk_to_eo).
// Each wave owns the spectrum points it finished for the multiply-accumulate over all six rows and both components: the fold order
// (trgsw.rs:290-299) holds trivially, no partial sums travel.  Buffer OWNERSHIP ping-pongs between the two waves: after a trade each wave owns the
// buffer it has just read -- its previous writer is done with it (its writes precede its arrival flag), its reader is this wave itself (DS
// instructions of a wave execute in order) -- so there is no "buffer free" synchronisation: ONE arrival / wait per trade, 3 per polynomial + 1 per
// inverse = 8 per step.  Same arithmetic DAG as the reference, every product and sum rounded on its own (-ffp-contract=off): bit-identical to
// k_bootstrap<11> (tests/test_gpu_configs.py::test_config5_*).
// LDS: the per-parity stage tables of passes 1-3 (16 KiB forward, 2 KiB inverse); twist / untwist / inverse pass-1 tables in global memory
// (a vector-memory read costs the SIMD's issue less than an LDS read does, and LDS is full: profiles/r05/vmem_issue.log).
// The accumulator lives in LDS as PARITY PLANES: coefficient c of a polynomial at word 1024 (c & 1) + (c >> 1) of its 8 KiB.  Wave H reads and
// updates the coefficients of parity H only (c = 2 (lane + 64 k) + H), and the rotated coefficients it gathers all have the parity of H - r
// (wave-uniform): every access of a wave goes to 64 CONSECUTIVE words of one plane -- no LDS bank conflict (the natural layout's stride of
// two words made every access two-way conflicted: 7.3 % of the LDS pipe's active cycles, profiles/r04/pmc_n2048_eo.json) -- and with the
// planes 4 KiB-aligned the address of a rotated coefficient is one add, one and-or from a per-polynomial lane constant.
// The kernel this one replaced (split by the TOP index bit, rounds 2-4) and every variant measured on the way are in profiles/HISTORY.md.
#pragma once

#include <type_traits>

#include "rtfhe_kernels_pair.hpp"

namespace rtfhe {

// twiddle table of the even / odd kernel, cplx units, everything [parity 0 | parity 1]
struct EoTw {
    static constexpr int TWIST = 0;                   // [2][8][64]  point i = 2 (lane + 64 m) + H                                   (global memory)
    static constexpr int P1 = TWIST + 2 * 8 * 64;     // [2][7][64]  pass 1: j-halfnn 256, 128, 64, entry layout of Geo<10>::TW_P1      (LDS from here ...
    static constexpr int P2 = P1 + 2 * 7 * 64;        // [2][7][8]   pass 2: j-halfnn 32, 16, 8
    static constexpr int P3 = P2 + 2 * 7 * 8;         // [2][8]      pass 3: j-halfnn 4 (4 entries), 2 (2 entries), 2 pad
    static constexpr int IP2 = P3 + 2 * 8;            // [2][7][8]   inverse pass 2
    static constexpr int IP3 = IP2 + 2 * 7 * 8;       // [2][8]      inverse pass 3                                                    ... to here)
    static constexpr int IP1 = IP3 + 2 * 8;           // [2][7][64]  inverse pass 1                                                    (global memory)
    static constexpr int IUNTW = IP1 + 2 * 7 * 64;    // [2][8][64]  untwist, times 2/N                                               (global memory)
    static constexpr int TOTAL = IUNTW + 2 * 8 * 64;
    static constexpr int LDS_CPLX = IP1 - P1;
};

struct EoLds {
    typedef Geo<10> G;   // geometry of a parity's 512-point sub-network
    // layout: [accumulators of all gates: 16 KiB each, so that every parity plane is 4 KiB-aligned][stage tables][per gate: rotation amounts, two
    // exchange buffer pairs, arrival counters]
    static constexpr size_t ACC = (size_t)2 * 2048 * 4;
    static constexpr size_t TW = (size_t)EoTw::LDS_CPLX * sizeof(cplx);
    static constexpr size_t XB = (size_t)2 * G::XSLOTS * sizeof(double);            // one wave's re + im exchange buffers: hold 512 cplx
    static constexpr size_t FLAGS = 16;       // two arrival counters per gate
    __host__ __device__ static constexpr size_t abar_bytes(int npad) { return ((size_t)npad * 2 + 15) / 16 * 16; }      // rotation amounts as u16
    __host__ __device__ static constexpr size_t rest_bytes(int npad) { return abar_bytes(npad) + 2 * XB + FLAGS; }
    __host__ __device__ static constexpr size_t gate_bytes(int npad) { return ACC + rest_bytes(npad); }
    __host__ __device__ static constexpr size_t bytes(int gates, int npad) { return TW + (size_t)gates * gate_bytes(npad); }
    // word of coefficient c (0 <= c < 2048) inside a polynomial's 2048 words
    __host__ __device__ static constexpr int plane_word(int c) { return ((c & 1) << 10) | (c >> 1); }
};

struct EoArgs {
    BootstrapArgs b;       // b.tw / b.bk unused
    const cplx* etw;       // [EoTw::TOTAL]
    const cplx* ebk;       // [n][2l rows][2 comp][2 waves][8][64]: k_bk_to_eo
};

// key spectra: device layout of k_bootstrap<11> ([n][row][comp][16][64]: lane v, register q <-> point (v << 4) | q) -> the layout the waves of
// k_bootstrap_eo hold their spectra in after the stage across them.  A parity's sub-network leaves lane v, register m with its output k = 8 v + m;
// the stage across the waves makes points 2k (sum) and 2k + 1 (difference).  Wave H finishes both for m = 4 H + j, j < 4: register j holds point
// 2k = (v << 4) | (8 H + 2 j), register 4 + j point 2k + 1.
__global__ __launch_bounds__(256) void k_bk_to_eo(const cplx* __restrict__ src, cplx* __restrict__ dst, size_t polys) {
    const size_t total = polys * 1024;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t g = idx >> 10;
        const int k = (int)(idx & 1023);                 // destination: (H, register, lane)
        const int H = k >> 9, m = (k >> 6) & 7, lane = k & 63;
        const int q = 8 * H + 2 * (m & 3) + (m >> 2);
        dst[idx] = src[g * 1024 + (size_t)q * 64 + lane];
    }
}

// pass 3 of a parity's sub-network, forward: i-halfnn 8 and 4 (twiddled, wave-uniform entries w[0..3] / w[4..5]), then this parity's half of the
// size-4 stage (spqlios-fft-impl.cpp:581-602): even points x0, x2 -> x0 + x2, x0 + (-x2); odd points x1, x3 -> x1 + x3, i (x1 - x3) = ((-j1) + j3, r1 + (-r3))
template <int R, bool ODD>
__device__ __forceinline__ void eo_fwd_pass3(double (&re)[R], double (&im)[R], const cplx* w) {
    fwd_stage_tw<R, 2, BOOT_TRIV && !ODD>(re, im, w);          // entry 0 of parity 0 is the reference's (1, 0): see fwd_stage_tw
    fwd_stage_tw<R, 1, BOOT_TRIV && !ODD>(re, im, w + 4);
#pragma unroll
    for (int m = 0; m < R; m += 2) {
        const double ra = re[m], rb = re[m + 1], ja = im[m], jb = im[m + 1];
        if (!ODD) { re[m] = ra + rb; re[m + 1] = ra + (-rb); im[m] = ja + jb; im[m + 1] = ja + (-jb); }
        else      { re[m] = ra + rb; re[m + 1] = (-ja) + jb; im[m] = ja + jb; im[m + 1] = ra + (-rb); }
    }
}
// ... inverse: this parity's half of the size-4 stage (:289-310): even x0, x2 -> x0 + x2, x0 + (-x2); odd x1, x3 -> x1 - i x3 = (r1 + j3, j1 + (-r3)),
// x1 + i x3 = (r1 + (-j3), j1 + r3); then i-halfnn 4 and 8
template <int R, bool ODD>
__device__ __forceinline__ void eo_inv_pass3(double (&re)[R], double (&im)[R], const cplx* w) {
#pragma unroll
    for (int m = 0; m < R; m += 2) {
        const double ra = re[m], rb = re[m + 1], ja = im[m], jb = im[m + 1];
        if (!ODD) { re[m] = ra + rb; re[m + 1] = ra + (-rb); im[m] = ja + jb; im[m + 1] = ja + (-jb); }
        else      { re[m] = ra + jb; re[m + 1] = ra + (-jb); im[m] = ja + (-rb); im[m + 1] = ja + rb; }
    }
    inv_stage_tw<R, 1, false, BOOT_TRIV && !ODD>(re, im, w + 4);
    inv_stage_tw<R, 2, false, BOOT_TRIV && !ODD>(re, im, w);
}

template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_bootstrap_eo(const EoArgs ea) {
    const TvGate tvs{};
#include "rtfhe_body_eo.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_eo(const LutArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const TvLut tvs = tv_lut(p, ea.b.fault);
#include "rtfhe_body_eo.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_many_eo(const ManyArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const TvMany tvs = tv_many(p, ea.b.fault);
#include "rtfhe_body_eo.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_enc_eo(const ManyArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const TvEnc tvs = tv_enc(p, ea.b.fault);
#include "rtfhe_body_eo.hpp"
}
// the rounded-decomposition twins of k_pbs_many_eo (E = false) and k_pbs_enc_eo (E = true): TvManyR / TvEncR, rtfhe_kernels.hpp
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES, bool E>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_round_eo(const ManyArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const auto tvs = tv_round<E>(p, ea.b.fault);
#include "rtfhe_body_eo.hpp"
}

}  // namespace rtfhe
