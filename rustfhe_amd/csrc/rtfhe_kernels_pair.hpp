// rtfhe_kernels_pair.hpp -- the bootstrap kernel with TWO WAVES PER GATE (N = 1024): the throughput shape.
//
// k_bootstrap gives a gate one wavefront.  With one gate per SIMD (the headline batch: 1024 gates on 1024 SIMDs) every
// SIMD then holds a single wave, and a lone wave issues one FP64 instruction per ~6.75 cycles where two waves sharing
// the SIMD reach one per ~5.4 (profiles/ubench/fp64_lds_issue_rates.log).  LDS (20 KiB of accumulator, exchange
// buffers and rotation amounts per gate) rules out more gates per CU, so here two waves share ONE gate's CMUX step.
// The arithmetic and its order are unchanged (see cmux_step for the reference citations):
//
//   side 0 (wave w, owns the b-poly)                       side 1 (wave w + GATES, owns the a-poly)
//   gather/decompose b-poly, transforms of rows 0..2       gather/decompose a-poly, transforms of rows 3..5   (spectra in VGPRs)
//   P: s0 = 0 + rows 0..2 of component 0    -> hand0
//   ------------------------------ hand-off 1 (the pair meets through its arrival flags in LDS) -----------------
//   Q: s1 = 0 + rows 0..2 of component 1    -> hand1       Q: s0 = hand0 + rows 3..5 of component 0  -> hand0
//   ------------------------------ hand-off 2 --------------------------------------------------------------------
//   s0 = hand0; inverse transform, += into the b-poly      R: s1 = hand1 + rows 3..5 of component 1; inverse, += into the a-poly
//
// * Fold order: every accumulator point sums rows 0, 1, ..., 5 from +0.0, exactly as the reference does
//   (trgsw.rs:290-299): the partial sums travel between the waves, products are never re-associated -> bit-identical.
// * Each side only ever reads and writes its OWN accumulator polynomial, so a side may run ahead into the next step's
//   gather and transforms; the two hand-offs per step order the partial sums only -- and only between the two waves of ONE gate (round 6:
//   flag_arrive / flag_wait, rtfhe_device.hpp; rounds 1-5 used the workgroup barrier at four gates per workgroup, which held the four gates in
//   lock step).  hand0 / hand1 are the (then idle) exchange buffers of side 0 / side 1: each is written only while its owner is between
//   transforms, in program order with the hand-offs.
// * Key rows go through a two-buffer register ring that runs ACROSS steps (each buffer is refilled right after its
//   multiply-accumulate retires; the last refills of a step fetch rows of the next).  Slot Q is the same code for both
//   sides, so the ring buffers are live in the same way on both paths at every control-flow merge -- the other
//   arrangements tried (per-side straight-line schedules, prefetch that only one side holds across a barrier) made the
//   register allocator spill 50-240 VGPRs, and scratch reloads share the vmcnt queue with the prefetches.
// * Priority schedule (see prio_point): a SIMD does not share itself evenly between two busy waves (one runs at ~0.9 of
//   its solo speed, the other on the leftovers; s_setprio selects which), so with fixed priorities one side races to each
//   hand-off and the SIMD then runs one wave; flipping side 0's priority twice per step makes both sides reach the
//   hand-offs together (8.16 -> 7.70 ms per 1024 gates).
// Measured (profiles/r01_pair): 7.70-7.75 ms per 1024 gates vs 8.69 ms for k_bootstrap's 4-wave shape, same outputs.
#pragma once

#include "rtfhe_kernels.hpp"

// What was tried on this kernel and measured slower (other priority schedules, a split-phase first hand-off, 8-byte hand-offs, 16-byte exchanges,
// the symmetric priority staircase, other wave placements) is recorded in profiles/HISTORY.md; the code below is what ships.

namespace rtfhe {

// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup-scope fence over ALL address
// spaces, i.e. s_waitcnt vmcnt(0): it would wait for the key rows prefetched across it.  Hand-offs here go through LDS.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Synchronisation of the TWO waves of one gate only, busy-polling form (k_bootstrap_pair's until round 6, still the four-wave and NTT kernels'
// at small workgroups; k_bootstrap_pair now uses the sleepy scalar-addressed flag_arrive / flag_wait of rtfhe_device.hpp at every size).  s_barrier is workgroup-wide although the four gates of a
// workgroup share nothing after start-up; the phase stamps show BOTH sides of a pair ~1.1 k cycles "at barrier 1", which looked like the pairs
// waiting for the slowest gate.  Here each side publishes an arrival counter in LDS after its hand-off stores and polls its partner's (DS
// instructions of a wave execute in order, so a partner that sees counter >= k also sees the stores issued before it; no fence, which would wait
// for the key rows in flight).  Identical outputs -- and no faster: 6.76 vs 6.74 ms per 1024 gates, 4.34 vs 4.37 at 512, 6.14 vs 6.20 at 768
// (profiles/r03/pair_flag_sync_ab.log).  The time at the barrier is the side's own hand-off stores draining, not skew between gates.
__device__ __forceinline__ void pair_sync(unsigned my_flag_addr, unsigned partner_flag_addr, unsigned k) {
    asm volatile("ds_write_b32 %0, %1" ::"v"(my_flag_addr), "v"(k) : "memory");
    unsigned v;
    do {
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(partner_flag_addr) : "memory");
        v = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
    } while ((int)(v - k) < 0);
}

// The two halves of pair_sync as separate calls (split phase): a wave publishes its arrival, does work that needs nothing from its partner, and only
// then waits -- the flag's LDS round trip lands under that work instead of idling the wave.
__device__ __forceinline__ void pair_arrive(unsigned my_flag_addr, unsigned k) {
    asm volatile("ds_write_b32 %0, %1" ::"v"(my_flag_addr), "v"(k) : "memory");
}
__device__ __forceinline__ void pair_wait(unsigned partner_flag_addr, unsigned k) {
    unsigned v;
    do {
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(partner_flag_addr) : "memory");
        v = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
    } while ((int)(v - k) < 0);
}

// pair_wait as ONE opaque statement: the spin loop lives inside the inline assembly, so the compiler sees straight-line code (a wait in the
// middle of a multiply-accumulate slot, with 200 registers live across it, otherwise becomes a loop header and the allocator spilled 88 of them)
__device__ __forceinline__ void pair_wait_opaque(unsigned partner_flag_addr, unsigned k) {
    unsigned v, t;
    asm volatile(
        "1:\n\t"
        "ds_read_b32 %0, %2\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %1, %0\n\t"
        "s_sub_i32 %1, %1, %3\n\t"
        "s_cmp_lt_i32 %1, 0\n\t"
        "s_cbranch_scc1 1b"
        : "=&v"(v), "=&s"(t)
        : "v"(partner_flag_addr), "s"(k)
        : "memory", "scc");
}

// ... and with the wave's priority raised to 3 behind the wait, inside the same statement (a separate s_setprio is one more scheduling boundary
// for the compiler: in k_bootstrap_eo at 256 registers eight of them per step cost 15 spilled registers)
__device__ __forceinline__ void pair_wait_opaque_prio3(unsigned partner_flag_addr, unsigned k) {
    unsigned v, t;
    asm volatile(
        "1:\n\t"
        "ds_read_b32 %0, %2\n\t"
        "s_waitcnt lgkmcnt(0)\n\t"
        "v_readfirstlane_b32 %1, %0\n\t"
        "s_sub_i32 %1, %1, %3\n\t"
        "s_cmp_lt_i32 %1, 0\n\t"
        "s_cbranch_scc1 1b\n\t"
        "s_setprio 3"
        : "=&v"(v), "=&s"(t)
        : "v"(partner_flag_addr), "s"(k)
        : "memory", "scc");
}

// the first row of a fold: the reference adds it to FrrSeries::zero() (trgsw.rs:290-299); +0.0 + x == x for every x except that
// it turns a -0.0 into +0.0, and the sign of a zero never reaches a torus word (see fwd_stage_tw in rtfhe_device.hpp)
template <int R>
__device__ __forceinline__ void mac_row_first(double (&sre)[R], double (&sim)[R], const cplx (&b)[R], const double (&re)[R], const double (&im)[R]) {
#pragma unroll
    for (int m = 0; m < R; m++) {
        const double ii = b[m].y * im[m], rr = b[m].x * re[m], ri = b[m].x * im[m], ir = b[m].y * re[m];
        sre[m] = rr - ii;
        sim[m] = ir + ri;
    }
}

template <int R>
__device__ __forceinline__ void mac_row(double (&sre)[R], double (&sim)[R], const cplx (&b)[R], const double (&re)[R], const double (&im)[R]) {
    // hadamard + fold-add, utils/src/spqlios.rs:204-222, hom_nand/src/trgsw.rs:290-299 (same operation order as cmux_step)
#pragma unroll
    for (int m = 0; m < R; m++) {
        const double ii = b[m].y * im[m], rr = b[m].x * re[m], ri = b[m].x * im[m], ir = b[m].y * re[m];
        sre[m] = sre[m] + (rr - ii);
        sim[m] = sim[m] + (ir + ri);
    }
}

struct PairLds {
    typedef Geo<10> G;
    static constexpr size_t TW = (size_t)G::TW_TOTAL * sizeof(cplx);
    static constexpr size_t XB = (size_t)2 * G::XSLOTS * sizeof(double);            // one wave's re + im exchange buffers
    static_assert(XB >= (size_t)G::P * sizeof(cplx), "an exchange buffer pair must hold one spectrum");
    static constexpr size_t FLAGS = 16;       // two arrival counters per gate (pair_sync), 16-byte aligned tail of the gate's region
    __host__ __device__ static constexpr size_t gate_bytes(int npad) { return (size_t)2 * G::N * 4 + (size_t)npad * 4 + 2 * XB + FLAGS; }
    __host__ __device__ static constexpr size_t bytes(int gates, int npad) { return TW + (size_t)gates * gate_bytes(npad); }
};

// GATES gates per workgroup, 2 * GATES waves: wave w serves gate (w % GATES) as side (w / GATES)
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_bootstrap_pair(const BootstrapArgs a) {
    const TvGate tvs{};
#include "rtfhe_body_pair.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_pair(const LutArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvLut tvs = tv_lut(p, a.fault);
#include "rtfhe_body_pair.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_many_pair(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvMany tvs = tv_many(p, a.fault);
#include "rtfhe_body_pair.hpp"
}
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_enc_pair(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvEnc tvs = tv_enc(p, a.fault);
#include "rtfhe_body_pair.hpp"
}
// the rounded-decomposition twins of k_pbs_many_pair (E = false) and k_pbs_enc_pair (E = true): TvManyR / TvEncR, rtfhe_kernels.hpp
template <int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int GATES, bool E>
__global__ __launch_bounds__(128 * GATES, 1) void k_pbs_round_pair(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const auto tvs = tv_round<E>(p, a.fault);
#include "rtfhe_body_pair.hpp"
}

}  // namespace rtfhe
