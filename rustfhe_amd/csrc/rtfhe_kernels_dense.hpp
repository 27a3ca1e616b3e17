// rtfhe_kernels_dense.hpp -- lvl0 dense layers: an integer matrix times a batch of TLWE rows as one exact contraction on the i8 matrix pipe.
//
//     out[g][o][c] = (accumulate ? out[g][o][c] : 0) + [c == n] bias[o] + sum_{i < I} W[o][i] x[g][i][c]   mod 2^32,   c = 0 .. n
//
// is an integer GEMM whose operand x[g] ([I] x [n + 1] words) is shared by all O outputs of a sample.  It is evaluated EXACTLY, the way
// k_key_switch_mm (rtfhe_kernels_ksmm.hpp) evaluates the key switch, with the roles turned round: here the CIPHERTEXT is split into byte limbs.
//
// Exactness.  A word is x = sum_j u_j 256^j with bytes u_j in [0, 255]; the pipe is fed s_j = u_j - 128 in [-128, 127] (one XOR with 0x80808080
// after the byte transpose) against the weights W[o][i] in [-128, 127].  v_mfma_i32_16x16x64_i8 accumulates sum_i W[o][i] s_j[i] in i32:
// |sum| <= I * 128 * 128 = I * 2^14 <= 2^30 at I = 65,536, the largest the interface accepts -- no overflow, of either sign.  What the offset
// drops is the same for every word of an output, 128 * 0x01010101 * sum_i W[o][i] mod 2^32: computed once at creation (corr,
// rtfhe_dense_weights_plan) and added back at recombination, with the bias on word n.  The four limb sums are recombined with shifts mod 2^32;
// u32 addition is associative and commutative, so the words equal the row-by-row wrapping sum.  Padded K (I up to a multiple of 64) holds zero
// bytes in W: the x rows read for it (clamped to row I - 1) never contribute, to the limb sums or to the correction.
//
// Operands.  A (the weights): [output tile = o / 16][K-step = i / 64][lane][16 B], lane 16 q + r of a tile holds W[16 tile + r][64 ks + 16 q + t]
// in byte t -- one KiB per wave-load, built once by k_dense_build; O x I bytes in all, read through the L1 by every wave of a CU (it is the
// small operand: 25 KB at 784 x 32).  B (the ciphertexts): lane 16 q + r of a word tile needs, for ITS word c, the 16 inputs 64 ks + 16 q + t:
// sixteen dword loads, each of which reads 64 contiguous bytes of four rows (coalesced along c; rows are only 4-byte aligned, so nothing wider
// is assumed), then a 4 x 4 byte transpose per four words (8 v_perm_b32) turns words into limb words.  No LDS, no scratch.
// D: lane holds word c = lane % 16 of outputs 4 (lane / 16) + r in register r: a store instruction writes 64 contiguous bytes of four rows.
//
// Tiling.  A wave owns DENSE_CT = 2 word tiles x OT = 1, 2 or 4 output tiles (16 accumulator registers per pair, 128 at most) and walks the
// K-steps of its slice; a workgroup is four waves on neighbouring words.  One pass over x[g] serves 16 OT outputs: O <= 64 reads x once, O = 512
// eight times, the passes of one sample being neighbours ON ONE XCD (the workgroup order below) so that all but the first MAY find x in that L2
// (the intent of the order; the reuse itself was not measured: no counter run was made).
// The launch rule -- OT, and whether I is cut into slices whose parts meet as wrapping u32 atomics -- is rtfhe_dense_launch_shape
// (rtfhe_dense_plan.cpp), nowhere else.
#pragma once

#include "rtfhe_kernels.hpp"
#include "rtfhe_dense_plan.h"

namespace rtfhe {

constexpr int DENSE_CT = RTFHE_DENSE_CT;
constexpr int DENSE_WAVES = 4;
constexpr int DENSE_BIAS_MAX = RTFHE_DENSE_BIAS_PER_LAUNCH;

struct DenseArgs {
    const uint4* wmat;       // [ceil(O / 16)][ksteps][64 lanes] x 16 B
    const uint32_t* corr;    // [O]
    const uint32_t* x;       // [count][I][n+1]
    uint32_t* out;           // [count][O][n+1]; slices > 1: zero or the accumulator on entry, every slice adds its part with a wrapping atomic
    int32_t count, O, I, n;
    int32_t o_first, o_end;  // the outputs of this launch: o_first a multiple of 16 OT
    int32_t groups, cwgs, ksteps, slices, steps;      // rtfhe_dense_shape of this launch
    int32_t accumulate, has_bias;
    uint32_t total;          // workgroups of work: count * cwgs * slices * groups
    // bias[o - o_first].  By value, so every launch -- one without a bias and one inside a captured graph too -- passes these 2 KiB of arguments.
    // The kernel indexes the array per lane: the compiler reads it from the kernarg segment with vector loads, which is why the kernels need no
    // scratch (ScratchSize 0 in the resource remarks; a build that copied the array to private memory would show there).
    uint32_t bias[DENSE_BIAS_MAX];
};
static_assert(sizeof(DenseArgs) <= 4096, "the arguments of one launch fit the 4 KiB kernarg limit");

typedef int dense_v4i __attribute__((ext_vector_type(4)));

// four words -> their four limb words (byte j of w0, w1, w2, w3 in limb j, least significant first), each byte minus 128
// (v_perm_b32: selector bytes 0 .. 3 pick from the SECOND operand, 4 .. 7 from the first)
__device__ __forceinline__ void dense_limbs(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, int& l0, int& l1, int& l2, int& l3) {
    const uint32_t lo01 = __builtin_amdgcn_perm(w1, w0, 0x05010400u), hi01 = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
    const uint32_t lo23 = __builtin_amdgcn_perm(w3, w2, 0x05010400u), hi23 = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
    l0 = (int)(__builtin_amdgcn_perm(lo23, lo01, 0x05040100u) ^ 0x80808080u);
    l1 = (int)(__builtin_amdgcn_perm(lo23, lo01, 0x07060302u) ^ 0x80808080u);
    l2 = (int)(__builtin_amdgcn_perm(hi23, hi01, 0x05040100u) ^ 0x80808080u);
    l3 = (int)(__builtin_amdgcn_perm(hi23, hi01, 0x07060302u) ^ 0x80808080u);
}

// grid: any multiple of 8 workgroups.  Workgroups go to the XCDs round-robin, so workgroup b takes the work items v, v + gridDim, ... with
// v = (b % 8) * gridDim / 8 + b / 8: consecutive items run on ONE XCD.  Item = ((g * cwgs + cw) * slices + slice) * groups + og, the output
// groups of one (sample, words, slice) innermost: they read the same x.
template <int OT>
__global__ __launch_bounds__(64 * DENSE_WAVES) void k_tlwe_dense(const DenseArgs a) {
    constexpr int CT = DENSE_CT;
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int words = a.n + 1, otiles = (a.O + 15) >> 4;
    const uint32_t nb = gridDim.x, first = (blockIdx.x & 7u) * (nb >> 3) + (blockIdx.x >> 3);
#pragma unroll 1
    for (uint32_t item = first; item < a.total; item += nb) {
        const int og = (int)(item % (uint32_t)a.groups);
        uint32_t rest = item / (uint32_t)a.groups;
        const int slice = (int)(rest % (uint32_t)a.slices); rest /= (uint32_t)a.slices;
        const int cw = (int)(rest % (uint32_t)a.cwgs), g = (int)(rest / (uint32_t)a.cwgs);
        const int c_base = (cw * DENSE_WAVES + wave) * 16 * CT;
        if (c_base > a.n) continue;                                      // (the words padded to whole workgroups; uniform per wave)
        const int tile0 = (a.o_first >> 4) + og * OT;
        const int ks_begin = slice * a.steps, ks_end = min(a.ksteps, ks_begin + a.steps);
        const uint32_t* xg = a.x + (size_t)g * (size_t)a.I * (size_t)words;
        int cl[CT];                                                      // this lane's word per tile, clamped for the loads: a word past n is never stored
#pragma unroll
        for (int ct = 0; ct < CT; ct++) cl[ct] = min(c_base + ct * 16 + r16, a.n);
        const uint4* wp[OT];                                             // an output tile past the last reads the last one: its rows are never stored
#pragma unroll
        for (int ot = 0; ot < OT; ot++) wp[ot] = a.wmat + (size_t)min(tile0 + ot, otiles - 1) * (size_t)a.ksteps * 64 + lane;
        dense_v4i acc[OT][CT][4];
#pragma unroll
        for (int ot = 0; ot < OT; ot++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[ot][ct][j] = (dense_v4i){0, 0, 0, 0};
#pragma unroll 1
        for (int ks = ks_begin; ks < ks_end; ks++) {
            const int i0 = ks * 64 + q * 16;
            dense_v4i wa[OT];
#pragma unroll
            for (int ot = 0; ot < OT; ot++) {
                const uint4 w = wp[ot][(size_t)ks * 64];
                wa[ot] = (dense_v4i){(int)w.x, (int)w.y, (int)w.z, (int)w.w};
            }
            uint32_t xw[CT][16];
            if (ks * 64 + 64 <= a.I) {                                   // whole K-step (uniform)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
#pragma unroll
                    for (int t = 0; t < 16; t++) xw[ct][t] = xg[(uint32_t)((i0 + t) * words + cl[ct])];
            } else {                                                     // the ragged last one: rows past I - 1 read row I - 1 against zero weights
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
#pragma unroll
                    for (int t = 0; t < 16; t++) xw[ct][t] = xg[(uint32_t)(min(i0 + t, a.I - 1) * words + cl[ct])];
            }
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                dense_v4i b[4];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    int l0, l1, l2, l3;
                    dense_limbs(xw[ct][4 * m], xw[ct][4 * m + 1], xw[ct][4 * m + 2], xw[ct][4 * m + 3], l0, l1, l2, l3);
                    b[0][m] = l0; b[1][m] = l1; b[2][m] = l2; b[3][m] = l3;
                }
#pragma unroll
                for (int ot = 0; ot < OT; ot++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[ot][ct][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(wa[ot], b[j], acc[ot][ct][j], 0, 0, 0);
            }
        }
        // D layout of a 16x16 i32 tile: lane holds column lane % 16 (the word), rows 4 (lane / 16) + r (the outputs) in register r
#pragma unroll
        for (int ot = 0; ot < OT; ot++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = (tile0 + ot) * 16 + 4 * q + r;
                if (o >= a.o_end) continue;
                const uint32_t fixed = slice == 0 ? a.corr[o] : 0u;
                const uint32_t bias = (slice == 0 && a.has_bias) ? a.bias[o - a.o_first] : 0u;
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    const int c = c_base + ct * 16 + r16;
                    if (c > a.n) continue;
                    const uint32_t s = (uint32_t)acc[ot][ct][0][r] + ((uint32_t)acc[ot][ct][1][r] << 8) + ((uint32_t)acc[ot][ct][2][r] << 16) +
                                       ((uint32_t)acc[ot][ct][3][r] << 24) + fixed + (c == a.n ? bias : 0u);
                    uint32_t* p = a.out + ((size_t)g * (size_t)a.O + (size_t)o) * (size_t)words + (size_t)c;
                    if (a.slices > 1) atomicAdd(p, s);
                    else *p = a.accumulate ? *p + s : s;
                }
            }
        }
    }
}

// the operand-order matrix from the caller's rows: raw int32 [O][I], entries already checked to lie in [-128, 127]; zero bytes where o >= O or i >= I
struct DenseBuildArgs {
    const int32_t* raw;
    uint4* wmat;
    int32_t O, I, ksteps, otiles;
};
__global__ __launch_bounds__(256) void k_dense_build(const DenseBuildArgs a) {
    const size_t total = (size_t)a.otiles * (size_t)a.ksteps * 64;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(idx & 63);
        const size_t rest = idx >> 6;
        const int ks = (int)(rest % (size_t)a.ksteps), tile = (int)(rest / (size_t)a.ksteps);
        const int o = tile * 16 + (lane & 15), i0 = ks * 64 + (lane >> 4) * 16;
        uint32_t w[4] = {0, 0, 0, 0};
        if (o < a.O)
            for (int t = 0; t < 16; t++)
                if (i0 + t < a.I) w[t >> 2] |= ((uint32_t)a.raw[(size_t)o * (size_t)a.I + (size_t)(i0 + t)] & 0xffu) << (8 * (t & 3));
        a.wmat[idx] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace rtfhe
