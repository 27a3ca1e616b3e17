// rtfhe_kernels_eo4.hpp -- N = 2048 with FOUR waves per gate: (polynomial, parity of the point index).  The shape for batches of up to two gates
// per CU, where k_bootstrap_eo leaves a SIMD one wave (or none) to issue from.
//
// k_bootstrap_eo (rtfhe_kernels_eo.hpp) splits every 1024-point transform over two waves by the parity of the point index; each of the two
// waves of a gate then runs all six forward rows and both inverse transforms of a CMUX step: 4.7 k instructions per wave and step, on ONE wave per
// SIMD when a CU holds one or two gates.  Here the step is also split the way k_bootstrap_pair (rtfhe_kernels_pair.hpp) splits it at N = 1024:
//
//   wave (side 0, parity H), owns the b-poly's points of parity H     wave (side 1, parity H), owns the a-poly's points of parity H
//   gather / decompose, rows 0..2 forward, trades with (0, 1 - H)     gather / decompose, rows 3..5 forward, trades with (1, 1 - H)
//   P: s0 = 0 + rows 0..2 of component 0     -> hand0
//   ------------------------------------------ hand-off 1 (the two sides of a parity) ------------------------------------------
//   Q: s1 = 0 + rows 0..2 of component 1     -> hand1                Q: s0 = hand0 + rows 3..5 of component 0   -> hand0
//   ------------------------------------------ hand-off 2 ----------------------------------------------------------------------
//   s0 = hand0; inverse transform (trade with (0, 1 - H)), += b-poly  R: s1 = hand1 + rows 3..5 of component 1; inverse, += a-poly
//
// * Every accumulator point sums rows 0, 1, ..., 5 from +0.0 in order (trgsw.rs:290-299): partial sums travel, products are never re-associated.
//   A wave holds BOTH outputs of half of the crossing butterflies (k_bootstrap_eo's half-width trade): side 0 and side 1 of a parity hold the same
//   spectrum points in the same registers, which is what the hand-offs need; the key is read in k_bk_to_eo's layout.
// * hand0 / hand1 are the exchange buffer a side's wave owns at that moment (ping-pong ownership between the parities, as in k_bootstrap_eo): idle
//   between a wave's last forward trade and its inverse.  Both sides of a parity make the same number of trades, so each knows which of the
//   other side's two buffers that is.
// * A side only ever reads and writes its OWN polynomial; its two parities publish their accumulator words to each other with one more
//   arrival / wait pair at the end of a step (k_bootstrap_eo gets that from the other component's trade).
// Same arithmetic DAG as the reference, every product and sum rounded on its own: bit-identical to k_bootstrap_eo and the one-wave kernel.
// MODE_EXTRACT / MODE_BLIND_ROTATE only: the fused key switch (MODE_GATE: RTFHE_KS_MM_MIN=0, foreign stream captures) stays on k_bootstrap_eo.
#pragma once

#include "rtfhe_kernels_eo.hpp"

// priorities at two gates per workgroup, where the two sides of a parity share a SIMD: side 1 at 1, side 0 at 2 from the start of a step and at 0 from
// a point on -- 1 = the end of its slot P, 2 = of its slot Q, 3 = its second exchange (k_bootstrap_pair's schedule), 4 = its last forward trade; 0 = no
// priorities.  Measured (profiles/r04/n2048_four_waves_priority_ab.log): 512 gates 8.12 (0) / 7.70-7.86 (1) / 7.83 (2) / 7.91 (3) / 7.84 (4) ms, 300
// gates 7.91 / 7.25-7.29 / 7.29 / 7.42 / 7.11 ms.
// (The wave-private exchanges as one 16-byte LDS access per complex value at one gate per workgroup, every wave alone on its SIMD: 5.82 -> 5.96 ms.)

namespace rtfhe {

struct Eo4Lds {
    typedef Geo<10> G;
    static constexpr size_t TW = EoLds::TW;
    static constexpr size_t XB = EoLds::XB;
    static constexpr size_t FLAGS = 32;       // per gate: 4 trade counters + 4 hand-off counters
    __host__ __device__ static constexpr size_t gate_bytes(int npad) { return (size_t)2 * 2048 * 4 + EoLds::abar_bytes(npad) + 4 * XB + FLAGS; }
    __host__ __device__ static constexpr size_t bytes(int gates, int npad) { return TW + (size_t)gates * gate_bytes(npad); }
};

template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_bootstrap_eo4(const EoArgs ea) {
    const TvGate tvs{};
#include "rtfhe_body_eo4.hpp"
}
template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_eo4(const LutArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const TvLut tvs = tv_lut(p, ea.b.fault);
#include "rtfhe_body_eo4.hpp"
}
template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_many_eo4(const ManyArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const TvMany tvs = tv_many(p, ea.b.fault);
#include "rtfhe_body_eo4.hpp"
}
template <int L, int BGBIT, int GATES>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_enc_eo4(const ManyArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const TvEnc tvs = tv_enc(p, ea.b.fault);
#include "rtfhe_body_eo4.hpp"
}
// the rounded-decomposition twins of k_pbs_many_eo4 (E = false) and k_pbs_enc_eo4 (E = true): TvManyR / TvEncR, rtfhe_kernels.hpp
template <int L, int BGBIT, int GATES, bool E>
__global__ __launch_bounds__(256 * GATES, 1) void k_pbs_round_eo4(const ManyArgs<EoArgs> p) {
    const EoArgs& ea = p.base;
    const auto tvs = tv_round<E>(p, ea.b.fault);
#include "rtfhe_body_eo4.hpp"
}

}  // namespace rtfhe
