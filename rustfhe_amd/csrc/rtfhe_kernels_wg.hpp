// rtfhe_kernels_wg.hpp -- latency-oriented variant of the bootstrap kernel: ONE GATE PER WORKGROUP.
//
// k_bootstrap (rtfhe_kernels.hpp) gives each gate one wavefront: best throughput once a launch has >= 4 gates per
// CU, but a gate then takes ~8.5 ms however few gates there are.  Dependency waves of a circuit (BASELINE config 4)
// and single hom_nand() calls are small; here the 8 waves of a 512-thread workgroup share one gate:
//
//   per CMUX step (same arithmetic, same operation order as the reference -- see cmux_step for citations):
//     F  waves 0..2l-3 : wave j gathers/decomposes digit polynomial j and runs its forward transform, spectrum -> LDS;
//        waves 2l-2..2l+1: the last two rows, each on TWO waves split by the parity of the point index (rtfhe_sub256.hpp): a wave gathers its
//                        parity's 256 points and runs their sub-network (4 points per lane); the size-2 stage across the parities is folded
//                        into the M phase's reads.  Every SIMD hosts one whole-row wave and one half-row wave from the start of the phase.
//                        (Round 1-3: the two rows were cut at their first exchange and handed from waves 2l-2, 2l-1 to waves 2l, 2l+1.)
//     -- barrier --
//     M  all 8 waves   : wave w owns points (lane << 3) | w of both accumulator spectra and runs their MAC chains
//                        over the 2l rows IN ROW ORDER (the reference's fold order), BK values prefetched at step start
//     -- barrier --
//     I  waves 0..3    : (component, parity): each inverse transform on two waves, again split by parity -- a lane reads the eight sums its
//                        four inputs need and applies the size-2 stage itself, so the waves trade nothing; truncate, += into the LDS accumulator
//     -- barrier --
//   key switch: each wave sums the rows of N/8 coefficients, partial sums reduced through LDS.
// Measured (profiles/r04/latency_parity_split_ab.log, same process, bit-identical): single gate 2.99 -> 2.88 ms (inverse split) -> 2.73 ms (rows
// split) -> 2.70 ms (half-row waves at priority 1 behind their second exchange).  The F phase is bound by instruction issue per SIMD (about 6.4
// cycles per instruction for the 800 a whole row plus a half row take): sixteen waves with EVERY row split -- three half rows per SIMD -- finish
// one after the other and end later (5.7 k cycles against 5.2 k; latency_sixteen_waves_ab.log).
//
// Only N = 1024 (R = 8 points per lane = 8 waves for the M phase; LDS 132 KiB).
#pragma once

#include "rtfhe_kernels.hpp"
#include "rtfhe_sub256.hpp"

// priority of the half-row waves during the F phase (they share a SIMD with a whole-row wave each: half the arithmetic, one more LDS round trip)
// ... and from its k-th exchange on (0 = never changed).  Measured (profiles/r04/latency_half_row_priority_ab.log): raised for the whole phase +7 % time;
// raised to 1 behind the second exchange -0.6 % (one gate) / -2 % (256 gates)

namespace rtfhe {

template <int LOGN, int L>
struct WgLds {
    typedef Geo<LOGN> G;
    static constexpr int NW = 8;
    // A spectrum row's slot is XSLOTS complex values wide (P of them the spectrum): the wave that produces the row uses the slot as its exchange
    // buffer first -- one 16-byte LDS access per complex value (in this latency-bound kernel half the LDS instructions are worth 1.6 % per phase,
    // profiles/r04/latency_16byte_exchanges_ab.log; in the throughput kernels they are not, see PAIR_X128) -- and the I phase's waves do the same.
    static constexpr int SROW = G::XSLOTS;
    static constexpr size_t TW = 0;
    static constexpr size_t ACC = TW + (size_t)G::TW_TOTAL * sizeof(cplx);
    static constexpr size_t SPEC = ACC + (size_t)2 * G::N * 4;                       // cplx[2l][SROW]  (also key-switch partials)
    static constexpr size_t SBUF = SPEC + (size_t)2 * L * SROW * sizeof(cplx);       // cplx[2][P]
    static constexpr size_t XBUF = SBUF + (size_t)2 * G::P * sizeof(cplx);           // cplx[4][Q4::XS]: exchange buffers of the half-row waves
    static constexpr size_t ABAR = XBUF + (size_t)4 * Q4::XS * sizeof(cplx);
    __host__ __device__ static constexpr size_t bytes(int npad) { return ABAR + (size_t)npad * 4; }
};

template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_bootstrap_wg(const BootstrapArgs a) {
    const TvGate tvs{};
#include "rtfhe_body_wg.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_pbs_wg(const LutArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvLut tvs = tv_lut(p, a.fault);
#include "rtfhe_body_wg.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_pbs_many_wg(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvMany tvs = tv_many(p, a.fault);
#include "rtfhe_body_wg.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ>
__global__ __launch_bounds__(512, 1) void k_pbs_enc_wg(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvEnc tvs = tv_enc(p, a.fault);
#include "rtfhe_body_wg.hpp"
}
// the rounded-decomposition twins of k_pbs_many_wg (E = false) and k_pbs_enc_wg (E = true): TvManyR / TvEncR, rtfhe_kernels.hpp
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ, bool E>
__global__ __launch_bounds__(512, 1) void k_pbs_round_wg(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const auto tvs = tv_round<E>(p, a.fault);
#include "rtfhe_body_wg.hpp"
}

}  // namespace rtfhe
