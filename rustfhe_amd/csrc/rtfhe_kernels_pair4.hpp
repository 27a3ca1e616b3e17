// rtfhe_kernels_pair4.hpp -- N = 1024 with FOUR waves per gate: (polynomial, parity of the point index).  k_bootstrap_eo4 (rtfhe_kernels_eo4.hpp)
// one size down, for batches and tails of more than one and up to three gates per CU, where k_bootstrap_pair leaves SIMDs one wave to issue from.
// (Three gates per workgroup: 168 registers per wave, the parity tables read pass by pass from LDS; four -- 128 registers, 22 spilled -- lose
// 12 % against k_bootstrap_pair's full round.)
//
//   wave (side 0, parity H), owns the b-poly's points of parity H     wave (side 1, parity H), owns the a-poly's points of parity H
//   gather / decompose, rows 0..2 forward, trades with (0, 1 - H)     gather / decompose, rows 3..5 forward, trades with (1, 1 - H)
//   P: s0 = 0 + rows 0..2 of component 0     -> hand0
//   ------------------------------------------ hand-off 1 (the two sides of a parity) ------------------------------------------
//   Q: s1 = 0 + rows 0..2 of component 1     -> hand1                Q: s0 = hand0 + rows 3..5 of component 0   -> hand0
//   ------------------------------------------ hand-off 2 ----------------------------------------------------------------------
//   s0 = hand0; inverse transform (trade with (0, 1 - H)), += b-poly  R: s1 = hand1 + rows 3..5 of component 1; inverse, += a-poly
//
// A wave runs one parity of a 512-point transform: the 256-point sub-network of rtfhe_sub256.hpp (4 points per lane, its 15 twiddles per direction
// resident in registers, its exchanges as 8-byte planes: at two waves per SIMD they beat the 16-byte form the latency kernel uses, 4.05 -> 3.89 ms), then the size-2 stage across the parities as a HALF-WIDTH trade -- the even wave finishes both outputs of the butterflies
// k = 4 v + m, m < 2, the odd wave m >= 2: it sends two complex values per lane and receives two -- so that both sides of a parity hold the same
// spectrum points in the same registers (register j < 2: point 2k, register 2 + j: point 2k + 1, k = 4 v + 2 H + j; key layout: k_bk_to_p4) and
// the partial sums travel lane to lane.  Buffers, flags, fold order, publishing of the accumulator words: as in k_bootstrap_eo4.
// Same arithmetic DAG as the reference, every product and sum rounded on its own: bit-identical to k_bootstrap_pair.
// MODE_EXTRACT / MODE_BLIND_ROTATE only: the fused key switch (MODE_GATE) stays on k_bootstrap_pair.
#pragma once

#include "rtfhe_kernels_pair.hpp"
#include "rtfhe_sub256.hpp"

// priorities at two gates per workgroup (the two sides of a parity share a SIMD): side 1 at 1, side 0 at 2 from the start of a step and at 0 from a
// point on -- 4 = its last forward trade (default), 5 = the end of the passes that use the exchange buffer, 6 = the end of its slot P; 0 = none;
// 1 = side 0 at 2 throughout.  Measured (profiles/r04/pair4_ab.log): 512 gates 4.34 (0) / 4.35 (1) / 4.06 (4) ms.
// (at three gates per workgroup, where the two sides of a parity do not always share a SIMD, the same schedule: 5.83 vs 6.04 ms per 768 gates without)

namespace rtfhe {

struct Pair4Args {
    BootstrapArgs b;       // b.tw: the staged table with the parity tables (Q4Tw) behind it; b.bk unused
    const cplx* p4bk;      // [n][2l rows][2 comp][2 waves][4][64]: k_bk_to_p4
};

struct Pair4Lds {
    static constexpr size_t XB = (size_t)Q4::XS * sizeof(cplx);       // one exchange buffer: 320 complex slots
    static constexpr size_t FLAGS = 32;                                // per gate: 4 trade counters + 4 hand-off counters
    __host__ __device__ static constexpr size_t abar_bytes(int npad) { return ((size_t)npad * 2 + 15) / 16 * 16; }
    __host__ __device__ static constexpr size_t gate_bytes(int npad) { return (size_t)2 * 1024 * 4 + abar_bytes(npad) + 4 * XB + FLAGS; }
    // three gates per workgroup (168 registers per wave): the parity tables are staged into LDS in front of the gates
    __host__ __device__ static constexpr size_t tw_bytes(int gates) { return gates >= 3 ? (size_t)Q4Tw::TOTAL * sizeof(cplx) : 0; }
    __host__ __device__ static constexpr size_t bytes(int gates, int npad) { return tw_bytes(gates) + (size_t)gates * gate_bytes(npad); }
};

// key spectra: device layout of the N = 1024 kernels ([n][row][comp][8][64]: lane v, register q <-> point (v << 3) | q) -> the layout the waves of
// k_bootstrap_pair4 hold their spectra in: wave H, register s, lane v <-> q = 4 H + 2 (s & 1) + (s >> 1)
__global__ __launch_bounds__(256) void k_bk_to_p4(const cplx* __restrict__ src, cplx* __restrict__ dst, size_t polys) {
    const size_t total = polys * 512;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t g = idx >> 9;
        const int k = (int)(idx & 511);                  // destination: (H, register, lane)
        const int H = k >> 8, s = (k >> 6) & 3, lane = k & 63;
        const int q = 4 * H + 2 * (s & 1) + (s >> 1);
        dst[idx] = src[g * 512 + (size_t)q * 64 + lane];
    }
}

template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_bootstrap_pair4(const Pair4Args pa) {
    const TvGate tvs{};
#include "rtfhe_body_pair4.hpp"
}
template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_pair4(const LutArgs<Pair4Args> p) {
    const Pair4Args& pa = p.base;
    const TvLut tvs = tv_lut(p, pa.b.fault);
#include "rtfhe_body_pair4.hpp"
}
template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_many_pair4(const ManyArgs<Pair4Args> p) {
    const Pair4Args& pa = p.base;
    const TvMany tvs = tv_many(p, pa.b.fault);
#include "rtfhe_body_pair4.hpp"
}
template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_enc_pair4(const ManyArgs<Pair4Args> p) {
    const Pair4Args& pa = p.base;
    const TvEnc tvs = tv_enc(p, pa.b.fault);
#include "rtfhe_body_pair4.hpp"
}
// the rounded-decomposition twins of k_pbs_many_pair4 (E = false) and k_pbs_enc_pair4 (E = true): TvManyR / TvEncR, rtfhe_kernels.hpp
template <int L, int BGBIT, int GATES, bool E>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_round_pair4(const ManyArgs<Pair4Args> p) {
    const Pair4Args& pa = p.base;
    const auto tvs = tv_round<E>(p, pa.b.fault);
#include "rtfhe_body_pair4.hpp"
}

}  // namespace rtfhe
