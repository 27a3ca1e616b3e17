// rtfhe_gate_frame.hpp -- the frame a bootstrap kernel puts around its step loop: the prologue (gate pre-step and mod switch into abar, acc =
// X^-bbar * testvec) and the epilogue (sample extract index 0 in place, the MODE_EXTRACT store, the fused identity key switch).  The fourteen kernel
// texts (the seven mirror bodies rtfhe_body_*.hpp and the seven exact-backend kernels of rtfhe_kernels_ntt*.hpp / rtfhe_kernels_xfft*.hpp) differ in
// how a gate's threads share these steps, and in nothing else; each helper takes that sharing as arguments -- which words this thread owns, how the
// owners of a polynomial meet -- and never a kernel's name.  The helpers are inlined and take scalars by value (a function taking a kernel's
// argument struct by reference changes its instruction order and scalar registers, rtfhe_body_pair.hpp).
//
// Who calls it: the families whose waves all share the a-polynomial (eo, eo4, pair4, k_bootstrap_ntt_halves) and k_bootstrap_xquad.  The other
// nine texts keep their own copy of these steps for now: written onto the helpers they compiled to one more LDS instruction or another register
// count than before (profiles/r29/README.md), and a clean-up does not get to move those.  A change to a step is made here AND in those nine.
//
// The barrier rule: a `sync` passed to a helper, and the sync inside gate_key_switch, is reached by every wave that shares it.  Idle waves of a
// partly filled workgroup and skipped gates shadow a live gate, run everything and store nothing: `live` guards stores only, never a sync.
//
// Included by rtfhe_kernels.hpp (never directly) behind the pieces the frame is built from: gate_io, gate_linear, the tv_* sources, mod_switch,
// many_extract, ks_accumulate.
#pragma once

namespace rtfhe {

// Pre-step (tfhe.rs:41-71) and mod switch (tfhe.rs:97, 107-108) of words i = t0, t0 + stride, ... <= n of the gate's two inputs into abar (32-bit
// words, or 16-bit where a family packs them): b floor, a_i rounded, both to [0, 2N).  Many-LUT kernels switch at SH + t and scale back
// (mod_switch); every other kernel keeps the literal k = 0 expression, see the note at tv_shift (rtfhe_kernels.hpp).
template <int LOGN, typename TV, typename AB>
__device__ __forceinline__ void gate_mask(const GateIo io, const TV tvs, int n, AB* abar, int t0, int stride) {
    constexpr int SH = 32 - LOGN - 1;
    for (int i = t0; i <= n; i += stride) {
        const uint32_t t = gate_linear(io.op, io.p0[i], io.p1[i], i == n);
        if constexpr (TV::MANY) abar[i] = (AB)mod_switch<SH>(t, i == n, tv_shift(tvs));
        else abar[i] = (AB)((i == n) ? (t >> SH) : ((t + (1u << (SH - 1))) >> SH));
    }
}

// Word c in [0, 2N) of the starting accumulator acc = X^-bbar * testvec (tfhe.rs:85, 98-106), b-polynomial at [0, N), a-polynomial at [N, 2N):
// b coefficient c is table word e = (c + bbar) mod 2N of the negacyclic extension; the a half is zero, or under ENC (an encrypted table) word
// (c - N + bbar) mod 2N = e ^ N of the row's a polynomial.  The callers keep their loop over the words they own.
template <int LOGN, typename TV, typename ROW>
__device__ __forceinline__ uint32_t acc_start(const TV, const ROW tv, int bbar, int c) {
    constexpr int N = 1 << LOGN;
    const int e = (c + bbar) & (2 * N - 1);
    if (c < N) return tv_word<LOGN>(tv, e);
    if constexpr (TV::ENC) return tv_word_a<LOGN>(tv, e ^ N);
    else return 0u;
}

// Sample extract index 0 (trlwe.rs:110-121) of the a-polynomial in place: a'_0 = a_0, a'_c = -a_{N-c}.  This thread holds words c0 + cstride k,
// k < K; sync() stands between the last read and the first write of the threads that share the polynomial (wave_lds_sync where one wave owns
// it, a barrier where several do).
template <int N, int K, typename SYNC>
__device__ __forceinline__ void extract_flip(uint32_t* apoly, int c0, int cstride, SYNC sync) {
    uint32_t av[K];
#pragma unroll
    for (int k = 0; k < K; k++) av[k] = apoly[c0 + cstride * k];
    sync();
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int c = c0 + cstride * k;
        apoly[(N - c) & (N - 1)] = (c == 0) ? av[k] : (0u - av[k]);
    }
}

// The MODE_EXTRACT store: the lvl1 sample(s) of gate number ge (batch-wide) into the batch key switch's operand (ext_slot), many_extract with
// one output unless the kernel is a many-LUT one.  This thread stores coefficients c0, c0 + step, ... < c1 and, if bl == 0 (many-LUT: 0 <= bl <
// 2^t), b'.  A gate kernel also zeroes words z0, z0 + zstride, ... <= n of its output row, which the batch key switch adds into; the many-LUT
// kernels' output rows are the key switch's own.  bpoly: the accumulator's b-polynomial; aprime: the index-0 sample the kernel has made of its
// a-polynomial (many-LUT: in place, aprime == bpoly + N, many_extract's layout).
template <int N, typename TV>
__device__ __forceinline__ void gate_extract_store(uint32_t* ext, uint32_t* out, const TV tvs, int n, int ge, const uint32_t* bpoly,
                                                   const uint32_t* aprime, int c0, int c1, int step, int bl, int z0, int zstride) {
    if constexpr (TV::MANY) many_extract<N>(ext, ge, tv_shift(tvs), bpoly, c0, c1, step, bl);
    else {      // many_extract at t = 0, spelled out: its c >= j test and second read are not always folded away
        for (int c = c0; c < c1; c += step) *ext_slot(ext, ge, c, N) = aprime[c];
        if (bl == 0) *ext_slot(ext, ge, N, N) = bpoly[0];
        for (int c = z0; c <= n; c += zstride) out[c] = 0u;
    }
}

// The fused identity key switch (tlwe.rs:43-73) of the sample (aprime[0..N), bpoly[0]) shared by W waves: wave w sums the rows of coefficients
// [w N/W, (w + 1) N/W); waves 1 .. W - 1 store their sums to `part` ([W - 1][KSQ][64] uint4), and behind sync() wave 0 adds them to the sums it
// holds in registers and writes b' - sum to out[0..n].  (The whole-workgroup kernels, eight waves a gate, meet otherwise -- every wave stores, all
// 512 threads sum one column each, b' read once before the extract -- and keep that form in their own text: rtfhe_body_wg.hpp,
// rtfhe_kernels_ntt_wg.hpp.)
template <int LOGN, int KS_T, int KS_BB, int KSQ, int W, typename SYNC>
__device__ __forceinline__ void gate_key_switch(const uint32_t* ksk, int ksw, uint32_t* out, int n, const uint32_t* bpoly, const uint32_t* aprime,
                                                uint4* part, int w, int lane, bool live, SYNC sync) {
    constexpr int N = 1 << LOGN;
    uint4 sum[KSQ];
    ks_accumulate<LOGN, KS_T, KS_BB, KSQ>(aprime, w * (N / W), (w + 1) * (N / W), ksk, ksw, sum, lane);
    part += lane;
    if (w != 0) {
        const int o = W == 2 ? 0 : w - 1;
#pragma unroll
        for (int q = 0; q < KSQ; q++) part[(o * KSQ + q) * 64] = sum[q];
    }
    sync();
    if (w == 0 && live) {
        const uint32_t bprime = bpoly[0];
#pragma unroll
        for (int q = 0; q < KSQ; q++) {
            uint32_t s[4] = {sum[q].x, sum[q].y, sum[q].z, sum[q].w};
#pragma unroll
            for (int o = 0; o < W - 1; o++) {
                const uint4 v = part[(o * KSQ + q) * 64];
                s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            }
            const int col = 4 * (lane + 64 * q);
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (col + e <= n) out[col + e] = ((col + e == n) ? bprime : 0u) - s[e];
        }
    }
}

}  // namespace rtfhe
