// rtfhe_kernels.hpp -- gfx950 kernels of the HomNAND hot path (one wavefront = one gate).
//
// Reference functions restated here (paths relative to the reference repo root):
//   gate pre-step            hom_nand/src/tfhe.rs:27-71
//   blind rotate             hom_nand/src/tfhe.rs:89-113
//   CMUX / external product  hom_nand/src/trgsw.rs:264-321, utils/src/spqlios.rs:204-222
//   gadget decomposition     utils/src/math.rs:300-326 (mask :542-560)
//   negacyclic rotate        utils/src/math.rs:85-132
//   sample extract           hom_nand/src/trlwe.rs:110-121
//   identity key switch      hom_nand/src/tlwe.rs:43-73
//
// Stated ONCE here for every kernel family: the digit-row loop of the external product (rtfhe_body_digit_rows.hpp, included by cmux_step below,
// mac_forward and auto_step) and the parked-row rule behind the batch key switch (park_row, k_rows_restore, beside ext_slot).
#pragma once

#include "rtfhe_device.hpp"

namespace rtfhe {

enum { OP_NAND = 0, OP_AND = 1, OP_OR = 2, OP_XOR = 3, OP_NOT = 4, OP_COPY = 5, OP_ANDNY = 6 };
enum { MODE_GATE = 0, MODE_BLIND_ROTATE = 1,
       MODE_EXTRACT = 2 };   // blind rotate + sample extract into `ext`, for the batch key switch that follows (rtfhe_kernels_ksmm.hpp)

struct BootstrapArgs {
    const cplx* tw;          // [Geo::TW_TOTAL] forward table then inverse table
    const cplx* bk;          // device layout [n][2l][2][R][64]
    const uint32_t* ksk;     // device layout [N*(t/2)*(base^2-1) + 1][ksw] (pairs of levels pre-summed, see ks_accumulate); last row all zero
    const uint32_t* in0;     // [count][n+1]
    const uint32_t* in1;     // [count][n+1] (may alias in0)
    uint32_t* out;           // MODE_GATE / MODE_EXTRACT: [count][n+1] (or the wire table);  MODE_BLIND_ROTATE: [count][2][N]
    uint32_t* ext;           // MODE_EXTRACT: lvl1 samples (a'[0..N), b') of the whole batch in the batch key switch's operand order (ext_slot
                             // below), gate number = ext_first + gate number within the launch; the gate's `out` row is ZEROED (the batch key
                             // switch adds its K-slices into it with wrapping atomics)
    int32_t count;
    int32_t op;
    int32_t n;
    int32_t steps;           // CMUX steps to run (= n for a real gate)
    int32_t mode;
    int32_t ksw;             // padded KSK row width in u32 (multiple of 4)
    int32_t npad;            // per-wave LDS words reserved for the mod-switched mask (>= n+1)
    int32_t ext_first;       // MODE_EXTRACT: the batch-wide number of this launch's first gate (segments of a batch share one sample buffer)
    // netlist mode (all null for a plain batch): gate g reads rows idx0[g], idx1[g] of in0 (the wire table), applies
    // ops[g] and writes row idx_out[g] of out
    const int32_t* ops;
    const int32_t* idx0;
    const int32_t* idx1;
    const int32_t* idx_out;
    int32_t num_wires;       // netlist mode: rows in the wire table; indices and opcodes are checked against it on the device
    int32_t* fault;          // netlist mode: set to 1 when a gate was skipped for an out-of-range index / unknown opcode
    unsigned long long* dbg;   // diagnostic builds only (RTFHE_WG_STAMPS): per-phase cycle sums of workgroup 0
};

// Where the split path keeps a batch's lvl1 samples between its two launches: the operand order of k_key_switch_mm (rtfhe_kernels_ksmm.hpp).
// Tiles of 16 gates, 16 N + 16 words each: [coefficient group kk / 4 (N / 16)][lane = 16 q + gate % 16][kk % 4] for coefficient
// c = q N/4 + kk, then the 16 b' words -- a wave of the key switch reads the four coefficients of its 64 (gate, q) rows as ONE contiguous
// KiB.  (Rows of N + 1 words, as the reference stores a TLWE sample, made that read 64 pieces of 16 B in 64 cache lines, re-read by every
// one of the 40 column groups: 10 GB through the L2 per 8,192 gates, the launch's bound until round 5.)  c == N addresses b'.
__device__ __forceinline__ size_t ext_tile_words(int N) { return 16 * (size_t)N + 16; }
__device__ __forceinline__ uint32_t* ext_slot(uint32_t* ext, int g, int c, int N) {
    uint32_t* tile = ext + (size_t)(g >> 4) * ext_tile_words(N);
    if (c == N) return tile + 16 * N + (g & 15);
    const int quarter = N >> 2, q = c / quarter, kk = c & (quarter - 1);
    return tile + ((((kk >> 2) * 64 + q * 16 + (g & 15)) << 2) | (kk & 3));
}

// The rule for an item that is skipped (an index out of range) in front of the batch key switch, stated once for every kernel family with an
// extract form.  The key switch writes every output row (k_key_switch_mm adds into a zeroed output), but a skipped item's row must keep its
// words: the item's threads PARK the row's n + 1 <= N words in the item's own, otherwise unused, sample slots (park_row; this thread moves
// words t0, t0 + stride, ... <= n), and k_rows_restore, launched behind the key switch (launch_key_switch_rows_restore, rtfhe_stages.hip),
// puts them back.  What the key switch makes of the parked words is overwritten.
template <int N, typename A>
__device__ __forceinline__ void park_row(const A& a, const uint32_t* out, int g, int t0, int stride) {      // a: the kernel's arguments, for a.ext and a.n
    if (!a.ext) return;      // not the extract form: nothing is stored and the row keeps its words anyway
    const uint32_t* keep = out + (size_t)g * ((size_t)a.n + 1);
    for (int c = t0; c <= a.n; c += stride) *ext_slot(a.ext, g, c, N) = keep[c];
}
// A wave per row.  Row g was skipped when one of its per_row entries of idx lies outside [0, bound): the rule of the kernel that parked it,
// checked again (the rotation: sel_idx, depth, n_sel; the multi-bit PBS: tv_idx, 1, n_tv).  idx null: no row was skipped.
struct RowsRestoreArgs {
    const int32_t* idx;      // [count][per_row]
    uint32_t* ext;           // the sample buffer the rows were parked in (ext_slot); read only
    uint32_t* out;           // [count][n+1], the key switch's output
    int32_t count, per_row, bound, n;
};
constexpr int ROWS_RESTORE_WAVES = 4;
template <int LOGN>
__global__ __launch_bounds__(64 * ROWS_RESTORE_WAVES) void k_rows_restore(const RowsRestoreArgs a) {
    constexpr int N = 1 << LOGN;
    const int lane = threadIdx.x & 63;
    const unsigned g = blockIdx.x * ROWS_RESTORE_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // wave-uniform; count + 3 < 2^32
    if (g >= (unsigned)a.count || !a.idx) return;
    const int32_t* idx = a.idx + (size_t)g * (unsigned)a.per_row;
    bool ok = true;
    for (int k = 0; k < a.per_row; k++) ok = ok && (unsigned)idx[k] < (unsigned)a.bound;
    if (ok) return;
    uint32_t* row = a.out + (size_t)g * (unsigned)(a.n + 1);
    for (int c = lane; c <= a.n; c += 64) row[c] = *ext_slot(a.ext, (int)g, c, N);
}

// gate pre-step on one TLWE word (a-part: isb = false, b-part: isb = true), hom_nand/src/tfhe.rs:27-71
__device__ __forceinline__ uint32_t gate_linear(int op, uint32_t x0, uint32_t x1, bool isb) {
    const uint32_t c8 = 0x20000000u;   // torus!(1/8), utils/src/math.rs:691-696
    const uint32_t c4 = 0x40000000u;   // torus!(2 * 1/8)
    switch (op) {
        case OP_NAND: return (isb ? c8 : 0u) - (x0 + x1);
        case OP_AND:  return (x0 + x1) - (isb ? c8 : 0u);
        case OP_OR:   return (x0 + x1) + (isb ? c8 : 0u);
        case OP_XOR:  return (x0 + x1) * 2u + (isb ? c4 : 0u);
        case OP_NOT:  return 0u - x0;
        case OP_ANDNY: return (x1 - x0) - (isb ? c8 : 0u);   // hom_and(-x0, x1), the second AND of hom_mux (tfhe.rs:34)
        default:      return x0;
    }
}

// Where gate g reads and writes.  Netlist gates with a wire index outside [0, num_wires) or an unknown opcode are
// skipped (ok = false: they run on row 0 and store nothing) and reported through *fault -- never dereferenced.
struct GateIo { const uint32_t* p0; const uint32_t* p1; uint32_t* out; int op; bool ok; };
__device__ __forceinline__ GateIo gate_io(const BootstrapArgs& a, int g) {
    const size_t w = (size_t)a.n + 1;
    GateIo io;
    if (a.idx0) {
        int i0 = a.idx0[g], i1 = a.idx1[g], o = a.idx_out[g];
        io.op = a.ops[g];
        const unsigned nw = (unsigned)a.num_wires;
        io.ok = (unsigned)i0 < nw && (unsigned)i1 < nw && (unsigned)o < nw && (unsigned)io.op <= (unsigned)OP_ANDNY;
        if (!io.ok) { i0 = 0; i1 = 0; o = 0; io.op = OP_COPY; if (a.fault) *a.fault = 1; }
        io.p0 = a.in0 + (size_t)i0 * w; io.p1 = a.in0 + (size_t)i1 * w; io.out = a.out + (size_t)o * w;
    } else {
        io.p0 = a.in0 + (size_t)g * w; io.p1 = a.in1 + (size_t)g * w; io.out = a.out + (size_t)g * w;
        io.op = a.op; io.ok = true;
    }
    return io;
}

// Where the accumulator of gate g starts: acc = X^{-bbar} * (tv, 0), coefficient c = tv_word<LOGN>(row, (c + bbar) mod 2N) (acc_start,
// rtfhe_gate_frame.hpp, states it once; the bodies that do not call the frame yet restate it).  Every mirror kernel family has one body
// (rtfhe_body_*.hpp) included into six __global__ entries that differ only in this source: k_bootstrap_* with TvGate, the gates' test vector
// (1/8, ..., 1/8) -- its row is always valid and its words are constants, so those kernels compile to what they were before the twins existed
// -- k_pbs_* with TvLut, the programmable bootstrap's caller-supplied tables (include/rtfhe.h), and the four further sources below.
struct TvGate {
    static constexpr bool MANY = false;      // one output per gate (k_pbs_many_*: several, see TvMany)
    static constexpr bool ENC = false;       // the a half starts at zero (k_pbs_enc_*: from an encrypted table, see TvEnc)
    static constexpr bool ROUNDED = false;   // the reference's gadget decomposition (k_pbs_round_*: rounded to nearest, see TvManyR)
    struct Row { __device__ __forceinline__ bool ok() const { return true; } };
};
__device__ __forceinline__ TvGate::Row tv_row(const TvGate&, int, int) { return TvGate::Row{}; }
template <int LOGN>
__device__ __forceinline__ uint32_t tv_word(const TvGate::Row&, int e) { return (e >> LOGN) ? 0xE0000000u : 0x20000000u; }

// the k_pbs_* kernels' arguments: the family's own struct, unchanged (its kernarg offsets stay those of the k_bootstrap_* twin), then the tables
template <typename A>
struct LutArgs {
    A base;
    const uint32_t* tv;        // [n_tv][N] test polynomials
    const int32_t* tv_idx;     // [count] the table of gate g (null: table 0 for every gate)
    int32_t n_tv;
};
// A gate whose index lies outside [0, n_tv) is skipped like a netlist gate with a bad wire (it runs on table 0 and stores nothing) and
// reported through *fault.  The index is read once per gate before the pre-step (and once more in k_bootstrap_pair_rr's epilogue).
struct TvLut {
    static constexpr bool MANY = false;
    static constexpr bool ENC = false;
    static constexpr bool ROUNDED = false;
    const uint32_t* tv; const int32_t* idx; int32_t n_tv; int32_t* fault;
    struct Row {
        const uint32_t* p; bool good;
        __device__ __forceinline__ bool ok() const { return good; }
    };
};
__device__ __forceinline__ TvLut::Row tv_row(const TvLut& t, int g, int N) {
    const int k = t.idx ? t.idx[g] : 0;
    const bool good = (unsigned)k < (unsigned)t.n_tv;
    if (!good && t.fault) *t.fault = 1;
    return TvLut::Row{t.tv + (size_t)(good ? k : 0) * N, good};
}
// where and whether gate g stores, for a body that derives it again after the step loop (k_bootstrap_pair_rr's epilogue): gate_io's rule,
// and for a programmable bootstrap also the table index's (an extra term in the gate kernel's own expression would change its code)
__device__ __forceinline__ GateIo gate_io(const BootstrapArgs& a, int g, const TvGate&) { return gate_io(a, g); }
__device__ __forceinline__ GateIo gate_io(const BootstrapArgs& a, int g, const TvLut& t) {
    GateIo io = gate_io(a, g);
    if (!tv_row(t, g, 0).ok()) io.ok = false;
    return io;
}
template <int LOGN>
__device__ __forceinline__ uint32_t tv_word(const TvLut::Row& r, int e) {      // the negacyclic extension: X^N = -1
    const uint32_t v = r.p[e & ((1 << LOGN) - 1)];
    return (e >> LOGN) ? 0u - v : v;
}
template <typename A>
__device__ __forceinline__ TvLut tv_lut(const LutArgs<A>& p, int32_t* fault) { return TvLut{p.tv, p.tv_idx, p.n_tv, fault}; }

// Many-LUT PBS (k_pbs_many_*, the third inclusion of every body): the tables of TvLut, whose rows interleave 2^t functions, and a mod switch
// rounded at SH + t and scaled back by 2^t, so that every rotation is a multiple of 2^t and coefficients 0 .. 2^t - 1 of the rotated
// accumulator hold the 2^t outputs (include/rtfhe.h: rtfhe_pbs_many_batch).  Such a kernel runs in MODE_EXTRACT only: sample extract
// index j (trlwe.rs:110-121) of every output goes to batch-wide row (gate << t) + j of the batch key switch's operand (many_extract).
template <typename A>
struct ManyArgs : LutArgs<A> {
    int32_t t;                 // log2 of the outputs per gate, 0 .. 3
};
struct TvMany : TvLut {
    static constexpr bool MANY = true;
    static constexpr bool ENC = false;
    int32_t t;
};
template <typename A>
__device__ __forceinline__ TvMany tv_many(const ManyArgs<A>& p, int32_t* fault) { return TvMany{{p.tv, p.tv_idx, p.n_tv, fault}, p.t}; }

// Encrypted tables (k_pbs_enc_*, the fourth inclusion of every body): the many-LUT PBS of TvMany started from a TRLWE encryption of the
// table instead of the trivial one, acc = X^{-bbar} * (tb, ta) (include/rtfhe.h: rtfhe_lut_create_encrypted).  The same ManyArgs, with tv
// pointing at [n_tv][2][N] (b then a, the TRLWE layout): a row is 2N words, tv_word gives its b half and tv_word_a its a half.  The bodies
// fill the a half under `if constexpr (ENC)` and keep their zero-filling expression for every other kernel.
struct TvEnc : TvMany {
    static constexpr bool ENC = true;
};
template <typename A>
__device__ __forceinline__ TvEnc tv_enc(const ManyArgs<A>& p, int32_t* fault) { return TvEnc{{{p.tv, p.tv_idx, p.n_tv, fault}, p.t}}; }
__device__ __forceinline__ TvLut::Row tv_row(const TvEnc& t, int g, int N) { return tv_row(static_cast<const TvLut&>(t), g, 2 * N); }
template <int LOGN>
__device__ __forceinline__ uint32_t tv_word_a(const TvLut::Row& r, int e) { return tv_word<LOGN>(TvLut::Row{r.p + (1 << LOGN), r.good}, e); }
// (the trivial a half of the gates' test vector: named by the discarded branches of the gate kernels, whose row type does not depend on a
// template parameter, never called)
template <int LOGN>
__device__ __forceinline__ uint32_t tv_word_a(const TvGate::Row&, int) { return 0u; }

// Rounded gadget decomposition (k_pbs_round_*, the fifth inclusion of every body, ENC = false / true): the many-LUT PBS of TvMany and the
// encrypted-table PBS of TvEnc with the decomposition's two constants replaced (decomp_add / decomp_xor, rtfhe_device.hpp); nothing else
// differs.  The same ManyArgs; a plain-table PBS in rounded mode is the many-LUT twin with t = 0 (include/rtfhe.h: rtfhe_set_decomposition).
struct TvManyR : TvMany {
    static constexpr bool ROUNDED = true;
};
struct TvEncR : TvEnc {
    static constexpr bool ROUNDED = true;
};
template <bool E, typename A>
__device__ __forceinline__ auto tv_round(const ManyArgs<A>& p, int32_t* fault) {
    if constexpr (E) return TvEncR{tv_enc(p, fault)};
    else return TvManyR{tv_many(p, fault)};
}

// The mod switch (tfhe.rs:97, 107-108) of one pre-stepped word at SH + k, scaled back by 2^k: b floor, a_i rounded, both to multiples of 2^k
// in [0, 2N).  k = tv_shift(tvs): t for many-LUT, 0 otherwise.  gate_mask (rtfhe_gate_frame.hpp) and the bodies that still carry their own
// pre-step call it under `if constexpr (MANY)` and keep the literal k = 0 expression for the gates' and the PBS's kernels: routed through this
// function (k a compile-time 0) those kernels' code changed by a few instructions.
__device__ __forceinline__ int tv_shift(const TvGate&) { return 0; }
__device__ __forceinline__ int tv_shift(const TvLut&) { return 0; }
__device__ __forceinline__ int tv_shift(const TvMany& t) { return t.t; }
template <int SH>
__device__ __forceinline__ uint32_t mod_switch(uint32_t x, bool isb, int k) {
    return isb ? ((x >> (SH + k)) << k) : (((x + (1u << (SH + k - 1))) >> (SH + k)) << k);
}

// Many-LUT epilogue: sample extract index j = 0 .. 2^t - 1 of the rotated accumulator acc (LDS: b-poly at [0, N), and at [N, 2N) the index-0
// sample a'_0[c] = a_0, -a_{N-c} the body has already put there) into the key switch's operand rows (ge << t) + j.  Index j is a'_0 times
// X^j, negacyclically: a'_j[c] = a_{j-c} for c <= j, -a_{N+j-c} above (trlwe.rs:110-121), i.e. a'_0[c - j] for c >= j and -a'_0[N + c - j]
// below; b'_j = b_j.  This thread stores coefficients c0, c0 + step, ... < c1 of every output and, if 0 <= bl < 2^t, b' of output bl.
template <int N>
__device__ __forceinline__ void many_extract(uint32_t* ext, int ge, int t, const uint32_t* acc, int c0, int c1, int step, int bl) {
    const int outs = 1 << t;
    for (int j = 0; j < outs; j++) {
        const int row = (ge << t) + j;
        for (int c = c0; c < c1; c += step) *ext_slot(ext, row, c, N) = c >= j ? acc[N + c - j] : 0u - acc[2 * N + c - j];
    }
    if (bl >= 0 && bl < outs) *ext_slot(ext, (ge << t) + bl, N, N) = acc[bl];
}

// One external product / CMUX on the wave-private accumulator in LDS.
//   CMUX = true : acc <- cross(bk_i, X^r * acc - acc) + acc      (trgsw.rs:319-321, tfhe.rs:103-110)
//   CMUX = false: acc <- cross(bk_i, acc)                          (trgsw.rs:264-306)
// accbuf: LDS u32 [2][N] (b then a).  bk_i: this TRGSW in device layout [2l][2][R][64] cplx.
// ROUNDED: the decomposition rounds to nearest with balanced digits (TvManyR): the k_pbs_round kernels, and the ROUNDED = true twins of the
// leveled kernels (k_cmux_tree, k_trgsw_rotate, k_cmux_net, k_external_product); every other caller leaves it false.
template <int LOGN, int L, int BGBIT, bool CMUX, bool DUAL = false, bool ROUNDED = false>
__device__ __forceinline__ void cmux_step(uint32_t* __restrict__ accbuf, int r, const cplx* __restrict__ bk_i,
                                          const cplx* __restrict__ twf, const cplx* __restrict__ twi, const cplx* __restrict__ twi_big,
                                          double* __restrict__ xbuf, int lane) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R;
    constexpr uint32_t MA = decomp_add(L, BGBIT, ROUNDED), MX = decomp_xor(L, BGBIT, ROUNDED);

    double s0re[R], s0im[R], s1re[R], s1im[R];
#pragma unroll
    for (int m = 0; m < R; m++) { s0re[m] = 0.0; s0im[m] = 0.0; s1re[m] = 0.0; s1im[m] = 0.0; }

#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const uint32_t* poly = accbuf + h * N;
        uint32_t u[2 * R];
#pragma unroll
        for (int mm = 0; mm < 2 * R; mm++) {
            const int c = lane + 64 * mm;
            const uint32_t own = poly[c];
            const uint32_t d = CMUX ? (rotated_coef<LOGN>(poly, c, r) - own) : own;
            u[mm] = (d + MA) ^ MX;
        }
        // the L digit rows of this polynomial, hadamard + fold-add from zero: the one body every external product includes
#define RTFHE_DIGIT_ROW(jj) (bk_i + (size_t)((h * L + jj) * 2) * R * 64 + lane)
#include "rtfhe_body_digit_rows.hpp"
    }

    // the 2/N input scaling of the reference (fft_processor_spqlios.cpp:158) is folded into the untwist twiddles
#pragma unroll 1
    for (int comp = 0; comp < 2; comp++) {
        double re[R], im[R];
#pragma unroll
        for (int m = 0; m < R; m++) {
            re[m] = comp ? s1re[m] : s0re[m];
            im[m] = comp ? s1im[m] : s0im[m];
        }
        fft_inverse<LOGN, DUAL>(re, im, twi, twi_big, xbuf, lane);
        uint32_t* poly = accbuf + comp * N;
#pragma unroll
        for (int m = 0; m < R; m++) {
            const int c = lane + 64 * m;
            const uint32_t x0 = trunc_to_torus(re[m]), x1 = trunc_to_torus(im[m]);
            if (CMUX) { poly[c] += x0; poly[c + P] += x1; }
            else      { poly[c] = x0;  poly[c + P] = x1; }
        }
    }
    wave_lds_sync();
}

// identity key switch of the lvl1 sample held as a'[0..N) in LDS (+ b'), hom_nand/src/tlwe.rs:43-73.
// ks_accumulate sums the selected rows for coefficients [i_begin, i_end) into per-lane uint4 accumulators (lane holds
// columns 4 (lane + 64 q) .. +3).  Rows are added in a different order than the reference's (i, l) loop: wrapping u32
// addition is commutative and associative, so the result is bit-identical.
//
// For the same reason the device copy of the key holds, per coefficient, the rows of KS_GROUP = 2 adjacent levels already
// summed: row (i, p, c) = KS[i][2p][d0] + KS[i][2p+1][d1] with c = d0 * base + d1 in 1 .. base^2 - 1 (k_ksk_combine).  A gate
// then gathers t/2 rows per coefficient of which 15/16 are non-zero instead of t rows of which 3/4 are: 9.8 MB instead of
// 15.6 MB per gate through the L2 (the key switch is L2-bandwidth bound: all gates of a launch reach it together), for a
// 2.5x larger table (156 MB, still resident in the Infinity Cache next to the bootstrapping key).
constexpr int KS_GROUP = 2;
__host__ __device__ constexpr int ks_dev_rows(int N, int t, int basebit) { return N * (t / KS_GROUP) * ((1 << (basebit * KS_GROUP)) - 1); }

template <int LOGN, int KS_T, int KS_BB, int KSQ, int KS_UI = 2 * KS_GROUP>
__device__ __forceinline__ void ks_accumulate(const uint32_t* __restrict__ aprime, int i_begin, int i_end,
                                              const uint32_t* __restrict__ ksk, int ksw, uint4 (&sum)[KSQ], int lane) {
    constexpr int N = 1 << LOGN;
    static_assert(KS_T % KS_GROUP == 0, "levels are grouped in pairs");
    constexpr int PT = KS_T / KS_GROUP, PBB = KS_BB * KS_GROUP, PBASE1 = (1 << PBB) - 1;
    constexpr uint32_t ROUND = (32 - KS_T * KS_BB) != 0 ? (1u << (32 - KS_T * KS_BB - 1)) : 0u;
    const int zero_row = ks_dev_rows(N, KS_T, KS_BB);
    // lanes past the end of a row re-read its last 16 bytes (branch-free); the columns they accumulate are never stored
    int idx[KSQ];
#pragma unroll
    for (int q = 0; q < KSQ; q++) { sum[q] = make_uint4(0, 0, 0, 0); idx[q] = min(lane + 64 * q, ksw / 4 - 1); }
    // KS_UI coefficients per iteration: KS_UI * PT rows (3 x 16 B per lane each) in flight per wave (4 by default: 192 VGPRs)
#pragma unroll 1
    for (int i = i_begin; i < i_end; i += KS_UI) {
        uint4 v[KS_UI][PT][KSQ];
#pragma unroll
        for (int k = 0; k < KS_UI; k++) {
            const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane((int)(aprime[i + k] + ROUND));
#pragma unroll
            for (int l = 0; l < PT; l++) {
                const uint32_t c = (u >> (32 - PBB * (l + 1))) & ((1u << PBB) - 1u);          // digits 2l, 2l+1 side by side
                const int row = c ? (((i + k) * PT + l) * PBASE1 + (int)c - 1) : zero_row;   // both digits 0 -> the shared all-zero row
                const uint4* p = reinterpret_cast<const uint4*>(ksk + (size_t)row * ksw);
#pragma unroll
                for (int q = 0; q < KSQ; q++) v[k][l][q] = p[idx[q]];
            }
        }
#pragma unroll
        for (int k = 0; k < KS_UI; k++)
#pragma unroll
            for (int l = 0; l < PT; l++)
#pragma unroll
                for (int q = 0; q < KSQ; q++) {
                    sum[q].x += v[k][l][q].x; sum[q].y += v[k][l][q].y; sum[q].z += v[k][l][q].z; sum[q].w += v[k][l][q].w;
                }
    }
}

// device key-switching key from the reference's [N][t][base-1] rows (padded to ksw words, + the all-zero row at `zero_src`):
// one block per output row (i, p, c)
struct KskCombineArgs {
    const uint32_t* raw;     // [N*t*(base-1) + 1][ksw]
    uint32_t* out;           // [ks_dev_rows + 1][ksw]; the last row is all zero
    int32_t N, ksw;
};
template <int KS_T, int KS_BB>
__global__ __launch_bounds__(256) void k_ksk_combine(const KskCombineArgs a) {
    constexpr int BASE1 = (1 << KS_BB) - 1, PT = KS_T / KS_GROUP, PBB = KS_BB * KS_GROUP, PBASE1 = (1 << PBB) - 1;
    const int rows = a.N * PT * PBASE1, zero_src = a.N * KS_T * BASE1;
    for (int r = blockIdx.x; r <= rows; r += gridDim.x) {
        uint32_t* dst = a.out + (size_t)r * a.ksw;
        if (r == rows) { for (int w = threadIdx.x; w < a.ksw; w += blockDim.x) dst[w] = 0u; continue; }
        const int c = r % PBASE1 + 1, ip = r / PBASE1, p = ip % PT, i = ip / PT;
        const int d0 = c >> KS_BB, d1 = c & BASE1;
        const int s0 = d0 ? ((i * KS_T + 2 * p) * BASE1 + d0 - 1) : zero_src;
        const int s1 = d1 ? ((i * KS_T + 2 * p + 1) * BASE1 + d1 - 1) : zero_src;
        const uint32_t* r0 = a.raw + (size_t)s0 * a.ksw;
        const uint32_t* r1 = a.raw + (size_t)s1 * a.ksw;
        for (int w = threadIdx.x; w < a.ksw; w += blockDim.x) dst[w] = r0[w] + r1[w];
    }
}

template <int LOGN, int KS_T, int KS_BB, int KSQ>
__device__ __forceinline__ void key_switch_wave(const uint32_t* __restrict__ aprime, uint32_t bprime,
                                                const uint32_t* __restrict__ ksk, int ksw, int n,
                                                uint32_t* __restrict__ out, int lane) {
    uint4 sum[KSQ];
    ks_accumulate<LOGN, KS_T, KS_BB, KSQ>(aprime, 0, 1 << LOGN, ksk, ksw, sum, lane);
#pragma unroll
    for (int q = 0; q < KSQ; q++) {
        const int col = 4 * (lane + 64 * q);
        const uint32_t s[4] = {sum[q].x, sum[q].y, sum[q].z, sum[q].w};
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (col + e <= n) out[col + e] = ((col + e == n) ? bprime : 0u) - s[e];
    }
}

}  // namespace rtfhe

// the prologue and epilogue of every bootstrap kernel, built from the pieces above
#include "rtfhe_gate_frame.hpp"

namespace rtfhe {

// one wave per SIMD (<= 4 waves per workgroup, N = 1024): separate real/imaginary exchange buffers (see exchange<>)
__host__ __device__ constexpr bool bootstrap_dual_xbuf(int logn, int waves) { return logn == 10 && waves <= 4; }
template <int LOGN>
__host__ __device__ constexpr size_t bootstrap_wave_lds_bytes(int npad, bool dual = false) {
    return (size_t)Geo<LOGN>::XSLOTS * sizeof(double) * (dual ? 2 : 1) + (size_t)2 * Geo<LOGN>::N * 4 + (size_t)npad * 4;
}
template <int LOGN>
__host__ __device__ constexpr size_t bootstrap_lds_bytes(int waves, int npad, bool dual = false) {
    return (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)waves * bootstrap_wave_lds_bytes<LOGN>(npad, dual);
}

// The hot-path kernel: pre-step, blind rotate (n CMUX steps), sample extract and identity key switch
// of `count` independent gates in ONE launch; wave w of block b owns gate b * WAVES + w from start to end.
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_bootstrap(const BootstrapArgs a) {
    const TvGate tvs{};
#include "rtfhe_body_wave.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_pbs(const LutArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvLut tvs = tv_lut(p, a.fault);
#include "rtfhe_body_wave.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_pbs_many(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvMany tvs = tv_many(p, a.fault);
#include "rtfhe_body_wave.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_pbs_enc(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const TvEnc tvs = tv_enc(p, a.fault);
#include "rtfhe_body_wave.hpp"
}
template <int LOGN, int L, int BGBIT, int KS_T, int KS_BB, int KSQ, int WAVES, bool E>
__global__ __launch_bounds__(64 * WAVES, 1) void k_pbs_round(const ManyArgs<BootstrapArgs> p) {
    const BootstrapArgs& a = p.base;
    const auto tvs = tv_round<E>(p, a.fault);
#include "rtfhe_body_wave.hpp"
}

// ------------------------------------------------------------------------------------------------
// stage-level kernels (one wave per item)
// ------------------------------------------------------------------------------------------------

struct FftArgs {
    const cplx* tw;
    const void* src;
    void* dst;
    int32_t count;
    int32_t dst_layout;   // forward: 0 = FrrSeries (Re[0..P) | Im[0..P)), 1 = device BK layout [R][64] cplx
    int32_t rows;         // dst_layout 1: 2l; source polys ordered [i][comp][row], device polys [i][row][comp]
    int32_t f64_io;       // forward: the source is double[count][N] (Spqlios_ifft); inverse: the result is double[count][N] (Spqlios_fft)
};

// source poly index (i, comp, row) -> device poly index (i, row, comp)
__host__ __device__ inline size_t bk_poly_remap(size_t g, int rows) {
    const size_t i = g / (2 * (size_t)rows), rem = g % (2 * (size_t)rows);
    const size_t comp = rem / rows, row = rem % rows;
    return (i * rows + row) * 2 + comp;
}

// Spqlios_ifft_i32 / _u32 (spqlios-wrapper.cpp:22-28): count polynomials of N int32 -> FrrSeries
template <int LOGN, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_fft_forward(const FftArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R;
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int idx = tid; idx < G::TW_DIR; idx += 64 * WAVES) tw[idx] = a.tw[idx];
    __syncthreads();
    double* xbuf = reinterpret_cast<double*>(tw + G::TW_DIR) + (size_t)wave * G::XSLOTS;
    for (int g = blockIdx.x * WAVES + wave; g < a.count; g += gridDim.x * WAVES) {
        double re[R], im[R];
        if (a.f64_io) {      // Spqlios_ifft (execute_reverse, fft_processor_spqlios.cpp:16-55): doubles in
            const double* src = reinterpret_cast<const double*>(a.src) + (size_t)g * N;
#pragma unroll
            for (int m = 0; m < R; m++) { re[m] = src[lane + 64 * m]; im[m] = src[lane + 64 * m + P]; }
        } else {
            const int32_t* src = reinterpret_cast<const int32_t*>(a.src) + (size_t)g * N;
#pragma unroll
            for (int m = 0; m < R; m++) { re[m] = (double)src[lane + 64 * m]; im[m] = (double)src[lane + 64 * m + P]; }
        }
        fft_forward<LOGN>(re, im, tw, xbuf, lane);
        if (a.dst_layout == 0) {
            double* dst = reinterpret_cast<double*>(a.dst) + (size_t)g * N;
#pragma unroll
            for (int m = 0; m < R; m++) { dst[G::pos3(lane, m)] = re[m]; dst[P + G::pos3(lane, m)] = im[m]; }
        } else {
            cplx* dst = reinterpret_cast<cplx*>(a.dst) + bk_poly_remap((size_t)g, a.rows) * P;
#pragma unroll
            for (int m = 0; m < R; m++) dst[m * 64 + lane] = make_double2(re[m], im[m]);
        }
    }
}

// Spqlios_fft_u32 (spqlios-wrapper.cpp:34-36): count FrrSeries -> polynomials of N torus words
template <int LOGN, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_fft_inverse(const FftArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R;
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int idx = tid; idx < G::TW_DIR; idx += 64 * WAVES) tw[idx] = a.tw[G::TW_DIR + idx];
    __syncthreads();
    double* xbuf = reinterpret_cast<double*>(tw + G::TW_DIR) + (size_t)wave * G::XSLOTS;
    for (int g = blockIdx.x * WAVES + wave; g < a.count; g += gridDim.x * WAVES) {
        const double* src = reinterpret_cast<const double*>(a.src) + (size_t)g * N;
        double re[R], im[R];   // 2/N is folded into the untwist twiddles
#pragma unroll
        for (int m = 0; m < R; m++) { re[m] = src[G::pos3(lane, m)]; im[m] = src[P + G::pos3(lane, m)]; }
        fft_inverse<LOGN>(re, im, tw, tw, xbuf, lane);
        if (a.f64_io) {      // Spqlios_fft (execute_direct, fft_processor_spqlios.cpp:108-153): doubles out, no truncation
            double* dst = reinterpret_cast<double*>(a.dst) + (size_t)g * N;
#pragma unroll
            for (int m = 0; m < R; m++) { dst[lane + 64 * m] = re[m]; dst[lane + 64 * m + P] = im[m]; }
            continue;
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.dst) + (size_t)g * N;
#pragma unroll
        for (int m = 0; m < R; m++) { dst[lane + 64 * m] = trunc_to_torus_wide(re[m]); dst[lane + 64 * m + P] = trunc_to_torus_wide(im[m]); }
    }
}

// FrrSeries layout <-> device BK layout, count polynomials (dir 0: FrrSeries -> device, 1: device -> FrrSeries)
template <int LOGN>
__global__ void k_bk_permute(const double* __restrict__ src, double* __restrict__ dst, size_t count, int dir, int rows) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P;
    const size_t total = count * P;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const size_t g = idx / P;
        const int k = (int)(idx % P);          // device index m * 64 + lane
        const int m = k >> 6, lane = k & 63;
        const int pos = G::pos3(lane, m);
        const size_t gd = bk_poly_remap(g, rows);   // g: FrrSeries-side index, gd: device-side index
        if (dir == 0) {
            dst[gd * N + 2 * k] = src[g * N + pos];
            dst[gd * N + 2 * k + 1] = src[g * N + P + pos];
        } else {
            dst[g * N + pos] = src[gd * N + 2 * k];
            dst[g * N + P + pos] = src[gd * N + 2 * k + 1];
        }
    }
}

// Spqlios_poly_mul (spqlios-wrapper.cpp:38-53): res = a (*) b mod X^N + 1 through the transform: both operands viewed as signed
// i32, forward transforms, complex pointwise product (aimbim = ai bi; arebim = ar bi; re = ar br - aimbim; im = ai br + arebim),
// inverse transform with truncation.  Every product and sum rounded on its own (the reference builds this loop with -Ofast and
// may contract it: off the gate path, parity there is +-1 LSB).
struct PolyMulArgs {
    const cplx* tw;
    const uint32_t* a;    // [count][N]
    const uint32_t* b;    // [count][N]
    uint32_t* res;        // [count][N]
    int32_t count;
};
template <int LOGN, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_poly_mul(const PolyMulArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, P = G::P, R = G::R;
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* tw = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int idx = tid; idx < G::TW_TOTAL; idx += 64 * WAVES) tw[idx] = a.tw[idx];
    __syncthreads();
    double* xbuf = reinterpret_cast<double*>(tw + G::TW_TOTAL) + (size_t)wave * G::XSLOTS;
    for (int g = blockIdx.x * WAVES + wave; g < a.count; g += gridDim.x * WAVES) {
        const int32_t* pa = reinterpret_cast<const int32_t*>(a.a) + (size_t)g * N;
        const int32_t* pb = reinterpret_cast<const int32_t*>(a.b) + (size_t)g * N;
        double ar[R], ai[R], br[R], bi[R];
#pragma unroll
        for (int m = 0; m < R; m++) { ar[m] = (double)pa[lane + 64 * m]; ai[m] = (double)pa[lane + 64 * m + P]; }
        fft_forward<LOGN>(ar, ai, tw, xbuf, lane);
#pragma unroll
        for (int m = 0; m < R; m++) { br[m] = (double)pb[lane + 64 * m]; bi[m] = (double)pb[lane + 64 * m + P]; }
        fft_forward<LOGN>(br, bi, tw, xbuf, lane);
#pragma unroll
        for (int m = 0; m < R; m++) {
            const double aimbim = ai[m] * bi[m], arebim = ar[m] * bi[m];
            const double t0 = ar[m] * br[m], t1 = ai[m] * br[m];
            ar[m] = t0 - aimbim;
            ai[m] = t1 + arebim;
        }
        fft_inverse<LOGN>(ar, ai, tw + G::TW_DIR, tw + G::TW_DIR, xbuf, lane);
        uint32_t* dst = a.res + (size_t)g * N;
#pragma unroll
        for (int m = 0; m < R; m++) { dst[lane + 64 * m] = trunc_to_torus_wide(ar[m]); dst[lane + 64 * m + P] = trunc_to_torus_wide(ai[m]); }
    }
}

struct ExtProdArgs {
    const cplx* tw;
    const cplx* bk;
    const int32_t* bk_index;   // [count]
    const uint32_t* trlwe;     // [count][2][N]
    uint32_t* out;             // [count][2][N]
    int32_t count;
};

template <int LOGN, int L, int BGBIT, int WAVES, bool ROUNDED>
__global__ __launch_bounds__(64 * WAVES, 1) void k_external_product(const ExtProdArgs a) {
    typedef Geo<LOGN> G;
    constexpr int N = G::N, R = G::R;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    cplx* tw = reinterpret_cast<cplx*>(smem);
    TwStage<LOGN>::stage(tw, a.tw, tid, 64 * WAVES);
    __syncthreads();
    const int g = blockIdx.x * WAVES + wave;
    if (g >= a.count) return;
    unsigned char* wbase = smem + (size_t)TwStage<LOGN>::LDS_CPLX * sizeof(cplx) + (size_t)wave * bootstrap_wave_lds_bytes<LOGN>(0);
    double* xbuf = reinterpret_cast<double*>(wbase);
    uint32_t* accbuf = reinterpret_cast<uint32_t*>(wbase + (size_t)G::XSLOTS * sizeof(double));
    for (int c = lane; c < 2 * N; c += 64) accbuf[c] = a.trlwe[(size_t)g * 2 * N + c];
    wave_lds_sync();
    const size_t trgsw_cplx = (size_t)2 * L * 2 * R * 64;
    cmux_step<LOGN, L, BGBIT, false, false, ROUNDED>(accbuf, 0, a.bk + (size_t)a.bk_index[g] * trgsw_cplx, TwStage<LOGN>::fwd(tw), TwStage<LOGN>::inv_small(tw), TwStage<LOGN>::inv_big(tw, a.tw), xbuf, lane);
    for (int c = lane; c < 2 * N; c += 64) a.out[(size_t)g * 2 * N + c] = accbuf[c];
}

struct KeySwitchArgs {
    const uint32_t* ksk;
    const uint32_t* tlwe1;   // [count][N+1]
    uint32_t* out;           // [count][n+1]
    int32_t count, n, ksw;
};

// the identity key switch of `count` lvl1 samples laid out for k_key_switch_mm (ext_slot), one wave each: a many-LUT PBS's batch key switch on a
// context without the matrix form of the key (RTFHE_KS_MM_MIN=0)
struct KeySwitchExtArgs {
    const uint32_t* ksk;
    uint32_t* ext;           // tiles of 16 samples (ext_slot); read only
    uint32_t* out;           // [count][n+1]
    int32_t count, n, ksw;
};
template <int LOGN, int KS_T, int KS_BB, int KSQ, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_key_switch_ext(const KeySwitchExtArgs a) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x * WAVES + wave;
    if (g >= a.count) return;
    uint32_t* ap = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * N;
    for (int c = lane; c < N; c += 64) ap[c] = *ext_slot(a.ext, g, c, N);
    wave_lds_sync();
    key_switch_wave<LOGN, KS_T, KS_BB, KSQ>(ap, *ext_slot(a.ext, g, N, N), a.ksk, a.ksw, a.n, a.out + (size_t)g * (a.n + 1), lane);
}

template <int LOGN, int KS_T, int KS_BB, int KSQ, int WAVES>
__global__ __launch_bounds__(64 * WAVES, 1) void k_key_switch(const KeySwitchArgs a) {
    constexpr int N = 1 << LOGN;
    extern __shared__ __align__(16) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.x * WAVES + wave;
    if (g >= a.count) return;
    uint32_t* ap = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * N;
    const uint32_t* src = a.tlwe1 + (size_t)g * (N + 1);
    for (int c = lane; c < N; c += 64) ap[c] = src[c];
    wave_lds_sync();
    key_switch_wave<LOGN, KS_T, KS_BB, KSQ>(ap, src[N], a.ksk, a.ksw, a.n, a.out + (size_t)g * (a.n + 1), lane);
}

}  // namespace rtfhe
