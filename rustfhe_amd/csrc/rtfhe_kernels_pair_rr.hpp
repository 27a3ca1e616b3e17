// rtfhe_kernels_pair_rr.hpp -- k_bootstrap_pair with FIVE or SIX gates on the four wave pairs of a CU (N = 1024): batches between whole rounds.
//
// k_bootstrap_pair fills a CU with four gates (eight waves at 256 registers: two per SIMD, the issue optimum) and a gate takes the whole launch,
// so a batch runs in rounds of 4 x CUs gates: 1,280 gates on 256 CUs cost a full round (6.4 ms) plus a round for the last 256 (2.7 ms on the
// latency kernel) although the arithmetic is 1.25 rounds.  Here a workgroup serves gc = 4 .. 6 gates on the same four pairs of waves by time
// slicing: the CMUX steps of its gates form one sequence of items t = step * gc + gate, and pair s works through the items t = s, s + 4, s + 8, ...
// Item t needs item t - gc (the same gate's previous step) -- at least one whole item earlier in ANOTHER pair's sequence when gc > 4 -- and
// everything a gate carries from step to step lives in LDS (its two polynomials, its rotation amounts), so a gate simply changes hands: each
// side publishes "step i of gate g done" in a flag of the gate after its update and waits for that flag before it gathers.  (A side only ever
// reads and writes its own polynomial: the flag is per gate AND side, written by one wave, waited for by one.)  The pairs free-run as in
// k_bootstrap_pair; the arithmetic and its order are that kernel's, operation for operation, so the outputs are bit-identical.
// Cost against k_bootstrap_pair: the side's own coefficients are read back from LDS at the gather (16 ds_read_b32 per wave and item) instead of
// staying in registers, and the rotation amounts are stored as 16-bit words so that six gates fit (163,328 of 163,840 bytes of LDS).
// A batch of 4 W < count <= 6 W gates on W CUs takes ceil(count / W) / 4 rounds instead of 2: on one box 1,025 gates 10.0 -> 8.6 ms, 1,280 gates
// 9.7 -> 8.4-8.7, 1,536 gates 10.7 -> 10.3-10.4, 2,304 gates 16.3 -> 15.0 (profiles/r06/pair_rr_sweep.log).  A SEVENTH gate fits once the big half
// of the inverse table is read from global memory instead (as at N = 2048); built, bit-identical, and no faster than a whole round plus a
// three-gates-per-CU tail (1,792 gates 12.1 against 12.2 ms, 1,600 gates 12.5 against 12.3): not kept.
#pragma once

#include "rtfhe_kernels_pair.hpp"

namespace rtfhe {

struct PairRrLds {
    typedef Geo<10> G;
    static constexpr int SLOTS = 4, GMAX = 6;
    static constexpr size_t TW = PairLds::TW, XB = PairLds::XB;
    static constexpr size_t SLOT = 2 * XB + 16;            // a pair's exchange / hand-off buffers and its two arrival counters
    static constexpr size_t DONE = 64;                     // [GMAX][2 sides] steps done, per gate and side
    __host__ __device__ static constexpr size_t gate_bytes(int npad) { return (size_t)2 * G::N * 4 + ((size_t)npad * 2 + 15) / 16 * 16; }
    __host__ __device__ static constexpr size_t bytes(int gates, int npad) { return TW + SLOTS * SLOT + DONE + (size_t)gates * gate_bytes(npad); }
};

// gridDim.x workgroups share a.count gates evenly (the first a.count % gridDim.x take one more); the host launches 4 <= gates per workgroup <= 6
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_bootstrap_pair_rr(const BootstrapArgs a) {
    const TvGate tvs{};
#include "rtfhe_body_pair_rr.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_pbs_pair_rr(const LutArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvLut tvs = tv_lut(p, a.fault);
#include "rtfhe_body_pair_rr.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_pbs_many_pair_rr(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvMany tvs = tv_many(p, a.fault);
#include "rtfhe_body_pair_rr.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_pbs_enc_pair_rr(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvEnc tvs = tv_enc(p, a.fault);
#include "rtfhe_body_pair_rr.hpp"
}
// the rounded-decomposition twins of k_pbs_many_pair_rr (E = false) and k_pbs_enc_pair_rr (E = true): TvManyR / TvEncR, rtfhe_kernels.hpp
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, bool E>
__global__ __launch_bounds__(512, 1) void k_pbs_round_pair_rr(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const auto tvs = tv_round<E>(p, a.fault);
#include "rtfhe_body_pair_rr.hpp"
}

}  // namespace rtfhe
