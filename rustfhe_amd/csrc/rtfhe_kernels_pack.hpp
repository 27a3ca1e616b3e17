// rtfhe_kernels_pack.hpp -- TFHE's public packing key switch: lvl0 samples into TRLWE rows (include/rtfhe.h: rtfhe_pack_batch[_dev]).
//
// One sample c = (a_0 .. a_{n-1}, b) becomes the TRLWE
//
//     S(c) = (b, 0) - sum_{i, j : d_ij != 0} PK[i][j][d_ij - 1] ,     d_ij = digit j of a_i (the digits of identity_key_switch)
//
// a sum of up to n t key rows of 2N words each: done as a gather, one output of P = N = 1024 samples would pull 1,024 * 635 * 8 rows of
// 8 KB -- 41 GB -- through the L2.  It is the batch key switch's problem (rtfhe_kernels_ksmm.hpp) with a wider key, and it is solved
// the same way, as an exact contraction on the i8 matrix pipe:
//
//     S[m][col] = sum_k  H[m][k] * PK[k][col] ,   k = (i, j, d),   H[m][k] = [ d_ij of sample m == d ]   (one-hot),   col < 2N
//
// with every key word split into four balanced base-256 limbs (k_pkmat_build), v_mfma_i32_16x16x64_i8 accumulating in i32
// (|sum| <= n t 128 = 786,432 at n = 768: no overflow) and the limb sums recombined with shifts mod 2^32: the same words as the
// row-by-row wrapping subtraction, in any order (u32 addition is associative and commutative).
//
// K order, as in k_key_switch_mm with n16 (n rounded up to a multiple of 16) in the place of N: K-step ks = 2 kk + h (kk < n16 / 4, h < 2);
// lane group q = lane / 16 owns coefficient i = q n16/4 + kk; the 16 operand bytes of a lane are t = 4 j' + d: level j = 4 h + j', digit
// value d (d = 0: a zero key row).  Coefficients i >= n are zero rows of the key, and their sample word reads as 0 (all digits 0).
// Key matrix in HBM: [colgroup = col / 16][ks][limb][lane][16 B], 2N / 16 column groups, n16 / 2 K-steps: N n16 256 bytes.
// A workgroup is PACK_WAVES waves of 64 samples each that walk the WHOLE K range of one column group (no K-slices: every word of S has one
// owner and is written with a plain store); the key chunks are staged through LDS once per workgroup, double-buffered, as round 5's kernel.
// The samples are read as they lie, plain rows [M][n+1]: a lane reads the four words of two chunks with four dword loads, a wave-load
// touches 64 cache lines -- what rtfhe_kernels_ksmm.hpp measured as the cost of plain rows.  Here the operand is 2.5 KB per sample against
// a 168 MB key matrix, and a tiling kernel in front would be a launch of its own for every call; DESIGN.md 5.11.
//
// k_pack_combine then forms out[g] = sum_p X^pos[p] (1 + X + .. + X^(rep-1)) S(c[g][p]) mod X^N + 1.  The factor W = 1 + .. + X^(rep-1) is
// common to all p, so a workgroup first gathers R = sum_p X^pos[p] S_p for one (g, half) -- one load per p and output word, the p range
// split over four thread groups and reduced through LDS -- and then applies W once as a difference of prefix sums: with F(x) the prefix
// sum of R's negacyclic extension (F(x) = Q[x] below N, Q[N-1] - Q[x-N] from N to 2N, period 2N since a whole period sums to 0),
// (W R)[c] = F(c) - F(c - rep).  u32 arithmetic is exact, so every order gives the same words.
#pragma once

#include "rtfhe_kernels.hpp"

namespace rtfhe {

typedef int pk_v4i __attribute__((ext_vector_type(4)));
typedef unsigned int pk_v4u __attribute__((ext_vector_type(4)));

constexpr int PACK_WAVES = 8;         // waves (of 64 samples) per workgroup of k_pack_ks_mm
constexpr int PACK_CHUNK = 4;         // K-steps per LDS chunk (= 2 coefficients per lane group)
constexpr int PACK_MT = 4;            // sample tiles (of 16) per wave

struct PackMmArgs {
    const uint32_t* tlwe;    // [M][n+1] plain lvl0 rows
    const uint4* kmat;       // [colgroups][n16/2 K-steps][4 limbs][64 lanes] x 16 B
    uint32_t* s;             // [M][2N]: -(sum of the selected key rows); b is added by k_pack_combine
    int32_t M, n, n16, colgroups;
    int32_t mgroups;         // workgroups along the samples: ceil(M / (64 * PACK_WAVES))
};

// grid: x = ((cg / 8) * mgroups + mgb) * 8 + cg % 8 (colgroups is a multiple of 8): the mgroups workgroups that walk one column group's panel
// are neighbours in dispatch order on one XCD, as in k_key_switch_mm
template <int KS_T, int KS_BB>
__global__ __launch_bounds__(64 * PACK_WAVES, 1) void k_pack_ks_mm(const PackMmArgs a) {
    static_assert(KS_T == 8 && KS_BB == 2, "operand packing: 4 levels x 4 digit values per 16-byte operand chunk");
    constexpr int MT = PACK_MT, W = PACK_WAVES, KC = PACK_CHUNK, NT = 64 * W;
    constexpr int CHUNK_V4 = KC * 4 * 64;                 // uint4 per chunk
    constexpr int PER_THREAD = CHUNK_V4 / NT;             // uint4 a thread stages per chunk
    static_assert(CHUNK_V4 % NT == 0, "whole uint4 per thread");
    constexpr uint32_t ROUND = 1u << (32 - KS_T * KS_BB - 1);
    const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rest = blockIdx.x >> 3;
    const int cg = (rest / a.mgroups) * 8 + (blockIdx.x & 7);
    if (cg >= a.colgroups) return;
    const int mg = (rest % a.mgroups) * W + wave;                               // this wave's group of 64 samples
    const int quarter = a.n16 / 4, ksteps = a.n16 / 2;
    // tiles of this wave that hold a sample at all (wave-uniform): the others are neither loaded nor multiplied
    const int tiles_w = __builtin_amdgcn_readfirstlane(min(MT, max(0, (a.M - mg * 64 + 15) >> 4)));
    // one-hot operands by digit byte: entry b = { 1 << 8 ((b >> 6) & 3), 1 << 8 ((b >> 4) & 3), 1 << 8 ((b >> 2) & 3), 1 << 8 (b & 3) }
    __shared__ pk_v4i onehot[256];
    __shared__ pk_v4i kbuf[2][CHUNK_V4];                  // [buffer][K-step of the chunk][limb][lane]
    for (int b = tid; b < 256; b += NT)
        onehot[b] = (pk_v4i){(int)(1u << (((b >> 6) & 3) * 8)), (int)(1u << (((b >> 4) & 3) * 8)), (int)(1u << (((b >> 2) & 3) * 8)), (int)(1u << ((b & 3) * 8))};
    pk_v4i acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[mt][j] = (pk_v4i){0, 0, 0, 0};
    // the row this lane supplies to tile mt (rows past the batch read the last one: they are multiplied but never written)
    const uint32_t* row[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) row[mt] = a.tlwe + (size_t)min((mg * MT + mt) * 16 + r16, a.M - 1) * ((size_t)a.n + 1);
    // The chunk of K-steps [ks0, ks0 + KC) of this column group's panel is CHUNK_V4 consecutive uint4: thread t stages uint4 t, t + NT, ...
    // through a buffer resource that ends with the panel.
    const __amdgpu_buffer_rsrc_t krsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint4*>(a.kmat + (size_t)cg * ksteps * 4 * 64), 0, ksteps * 4096, 0x00020000);
    const int tid16 = tid * 16;
    pk_v4u stage[PER_THREAD];
    auto fetch_chunk = [&](int ks0) {
        const int soff = __builtin_amdgcn_readfirstlane(ks0 * 4096);
#pragma unroll
        for (int p = 0; p < PER_THREAD; p++) stage[p] = __builtin_amdgcn_raw_buffer_load_b128(krsrc, tid16 + p * NT * 16, soff, 0);
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PER_THREAD; p++) kbuf[buf][tid + p * NT] = (pk_v4i){(int)stage[p].x, (int)stage[p].y, (int)stage[p].z, (int)stage[p].w};
    };
    const int nchunks = quarter * 2 / KC;                 // even: quarter is a multiple of 4
    fetch_chunk(0);
    store_chunk(0);
    __syncthreads();
    uint32_t aw[MT][4];
#pragma unroll 1
    for (int c = 0; c < nchunks; c++) {
        const int kk2 = c * (KC / 2);                     // first of the chunk's two coefficients (per lane group)
        if (c + 1 < nchunks) fetch_chunk((c + 1) * KC);   // the next chunk: in flight under this chunk's multiplies
        if ((c & 1) == 0) {                               // sample words of four coefficients at a time (two chunks); past n: word 0
            const int i0 = q * quarter + kk2;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                if (mt < tiles_w) {
#pragma unroll
                    for (int e = 0; e < 4; e++) aw[mt][e] = i0 + e < a.n ? row[mt][i0 + e] : 0u;
                }
            }
        }
        const pk_v4i* kb = kbuf[c & 1] + lane;
#pragma unroll
        for (int t = 0; t < KC; t++) {                    // K-step 2 kk + h: coefficient e = t / 2 of the chunk, byte h = t % 2
            const int h = t & 1;
            pk_v4i b[4];
#pragma unroll
            for (int j = 0; j < 4; j++) b[j] = kb[(t * 4 + j) * 64];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                if (mt < tiles_w) {
                    const uint32_t w0 = (c & 1) ? aw[mt][2 + (t >> 1)] : aw[mt][t >> 1];
                    const uint32_t byte8 = ((w0 + ROUND) >> (24 - 8 * h)) & 0xffu;         // levels 4h .. 4h+3, most significant first
                    const pk_v4i av = onehot[byte8];
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[mt][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, b[j], acc[mt][j], 0, 0, 0);
                }
            }
        }
        if (c + 1 < nchunks) store_chunk((c + 1) & 1);    // (that buffer's last readers finished chunk c - 1 before the barrier of iteration c - 1)
        __syncthreads();
    }
    // D layout of a 16x16 i32 tile: lane holds column lane % 16, rows 4 (lane / 16) + r in register r
    const int col = cg * 16 + r16;
    const size_t width = (size_t)a.colgroups * 16;
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = (mg * MT + mt) * 16 + 4 * q + r;
            if (m >= a.M) continue;
            const uint32_t s = (uint32_t)acc[mt][0][r] + ((uint32_t)acc[mt][1][r] << 8) + ((uint32_t)acc[mt][2][r] << 16) + ((uint32_t)acc[mt][3][r] << 24);
            a.s[(size_t)m * width + col] = 0u - s;
        }
    }
}

// key matrix from the rows as uploaded: raw[((i * t + j) * (base - 1) + d - 1)][2N] (b then a)  ->  signed byte limbs in operand order
struct PkMatArgs {
    const uint32_t* raw;     // [n * t * (base-1)][2N]
    uint4* kmat;
    int32_t n, n16, colgroups;
};
template <int KS_T, int KS_BB>
__global__ __launch_bounds__(256) void k_pkmat_build(const PkMatArgs a) {
    const int ksteps = a.n16 / 2, quarter = a.n16 / 4;
    const size_t total = (size_t)a.colgroups * ksteps * 4 * 64, width = (size_t)a.colgroups * 16;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(idx & 63), limb = (int)((idx >> 6) & 3);
        const size_t rest = idx >> 8;
        const int ks = (int)(rest % ksteps), cg = (int)(rest / ksteps);
        const int col = cg * 16 + (lane & 15), q = lane >> 4, kk = ks >> 1, h = ks & 1, i = q * quarter + kk;
        uint32_t out[4] = {0, 0, 0, 0};
        if (i < a.n) {
            for (int t = 0; t < 16; t++) {
                const int l = 4 * h + (t >> 2), d = t & 3;
                if (d == 0) continue;
                uint32_t w = a.raw[((size_t)(i * KS_T + l) * ((1 << KS_BB) - 1) + (d - 1)) * width + col];
                int32_t s = 0;
                for (int j = 0; j <= limb; j++) {          // balanced base-256 digits, least significant first; the last carry drops mod 2^32
                    s = (int32_t)(int8_t)(w & 0xffu);
                    w = (w - (uint32_t)s) >> 8;
                }
                out[t >> 2] |= ((uint32_t)s & 0xffu) << (8 * (t & 3));
            }
        }
        a.kmat[idx] = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

constexpr int PACK_POS_MAX = 512;     // positions one k_pack_combine launch carries in its arguments
constexpr int PACK_CT = 1024;         // threads of a k_pack_combine workgroup: PACK_PS groups of 256, one group per slice of the p range
constexpr int PACK_PS = 4;

struct PackCombineArgs {
    const uint32_t* s;       // [count * P][2N] from k_pack_ks_mm
    const uint32_t* tlwe;    // [count * P][n+1]: b is word n
    uint32_t* out;           // [count][2][N]
    int32_t P, n, rep;
    int32_t p0, np;          // this launch adds samples p0 .. p0 + np - 1 of every output (np <= PACK_POS_MAX) ...
    int32_t accumulate;      // ... to what out holds (1: a later launch of the same call) or to zero (0)
    int32_t pos[PACK_POS_MAX];     // pos[p0 + k], each in [0, 2N)
};

// one workgroup per (output g, half h); every word of out[g][h] has one owner in the last phase and is written with a plain store
template <int LOGN>
__global__ __launch_bounds__(PACK_CT, 1) void k_pack_combine(const PackCombineArgs a) {
    constexpr int N = 1 << LOGN, M2 = 2 * N - 1, WPT = N / 256, EPT = N / PACK_CT;
    static_assert(N % PACK_CT == 0, "whole words per thread");
    __shared__ uint32_t red[PACK_PS][N];      // partial gathers, then red[0] = R and its prefix sums
    const int tid = threadIdx.x, l256 = tid & 255, slice = tid >> 8;
    const int g = blockIdx.x >> 1, h = blockIdx.x & 1;
    uint32_t acc[WPT];
#pragma unroll
    for (int j = 0; j < WPT; j++) acc[j] = 0;
#pragma unroll 4
    for (int k = slice; k < a.np; k += PACK_PS) {
        const int shift = a.pos[k];
        const size_t m = (size_t)g * a.P + a.p0 + k;
        const uint32_t* sp = a.s + m * 2 * N + (size_t)h * N;
#pragma unroll
        for (int j = 0; j < WPT; j++) {
            const int u = (l256 + 256 * j - shift) & M2, uu = u & (N - 1);
            uint32_t v = sp[uu];
            if (h == 0 && uu == 0) v += a.tlwe[m * ((size_t)a.n + 1) + a.n];      // S.b[0] carries the sample's b
            acc[j] += u < N ? v : 0u - v;
        }
    }
#pragma unroll
    for (int j = 0; j < WPT; j++) red[slice][l256 + 256 * j] = acc[j];
    __syncthreads();
    uint32_t x[EPT];
#pragma unroll
    for (int j = 0; j < EPT; j++) {
        const int c = tid + PACK_CT * j;
        x[j] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    }
    uint32_t* o = a.out + ((size_t)g * 2 + h) * N;
    if (a.rep == 1) {
#pragma unroll
        for (int j = 0; j < EPT; j++) {
            const int c = tid + PACK_CT * j;
            o[c] = (a.accumulate ? o[c] : 0u) + x[j];
        }
        return;
    }
    // inclusive prefix sums of R in red[0] (each thread reads only its own words of red[0] above, so the first barrier below orders the overwrite)
    uint32_t* Q = red[0];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EPT; j++) Q[tid + PACK_CT * j] = x[j];
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        uint32_t t[EPT];
#pragma unroll
        for (int j = 0; j < EPT; j++) {
            const int c = tid + PACK_CT * j;
            t[j] = c >= off ? Q[c - off] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EPT; j++) Q[tid + PACK_CT * j] += t[j];
        __syncthreads();
    }
    const uint32_t total = Q[N - 1];
#pragma unroll
    for (int j = 0; j < EPT; j++) {
        const int c = tid + PACK_CT * j, lo = (c - a.rep) & M2;      // F(c) - F(c - rep), F of period 2N
        const uint32_t f_lo = lo < N ? Q[lo] : total - Q[lo - N];
        o[c] = (a.accumulate ? o[c] : 0u) + Q[c] - f_lo;
    }
}

}  // namespace rtfhe
