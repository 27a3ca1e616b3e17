// rtfhe_kernels_seeded.hpp -- k_seeded_expand: a seeded object (public seed, first row, the b polynomials) into the project's full layout
// [rows / group][2][group][N] in one launch (include/rtfhe.h, "seeded ciphertexts"; the CPU form and oracle: rtfhe_seeded_expand in
// rtfhe_seeded.cpp).  A lane owns one 64-byte block (row r, block c): it computes the ChaCha20 block of stream first_row + r, counter c, stores
// the 16 words at the row's a position and copies the matching 64 bytes of b to the row's b position.  Integer only, no LDS, nothing allocated.
// The seed rides in the kernel arguments: a stream capture bakes it in.
#pragma once

#include <hip/hip_runtime.h>

#include "rtfhe_chacha.hpp"

namespace rtfhe {

struct SeededArgs {
    uint32_t seed[8];
    uint64_t first_row;
    const uint32_t* b;      // [rows][N]
    uint32_t* out;          // [rows / group][2][group][N]
    uint32_t blocks;        // rows * N / 16, below 2^31 (rtfhe_seeded_plan)
    int32_t logn;           // log2 N, 4 .. 11
    int32_t group;
};

constexpr int SEEDED_THREADS = 256;

__global__ __launch_bounds__(SEEDED_THREADS) void k_seeded_expand(SeededArgs a) {
    const uint32_t t = blockIdx.x * SEEDED_THREADS + threadIdx.x;
    if (t >= a.blocks) return;
    const int lb = a.logn - 4;
    const uint32_t r = t >> lb, c = t & ((1u << lb) - 1u);
    const uint32_t g = r / (uint32_t)a.group, j = r - g * (uint32_t)a.group;
    // (a vector type of the compiler's own: each access below stays one aligned 16-byte instruction)
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const u32x4* src = reinterpret_cast<const u32x4*>(a.b + ((size_t)r << a.logn) + (size_t)c * 16);
    const size_t bpos = (((size_t)g * 2 * (size_t)a.group + j) << a.logn) + (size_t)c * 16;
    u32x4* dst_b = reinterpret_cast<u32x4*>(a.out + bpos);
    u32x4* dst_a = reinterpret_cast<u32x4*>(a.out + bpos + ((size_t)a.group << a.logn));
    const u32x4 b0 = src[0], b1 = src[1], b2 = src[2], b3 = src[3];
    uint32_t ks[16];
    chacha_block(a.seed, (uint64_t)c, a.first_row + (uint64_t)r, ks);
    dst_a[0] = u32x4{ks[0], ks[1], ks[2], ks[3]};
    dst_a[1] = u32x4{ks[4], ks[5], ks[6], ks[7]};
    dst_a[2] = u32x4{ks[8], ks[9], ks[10], ks[11]};
    dst_a[3] = u32x4{ks[12], ks[13], ks[14], ks[15]};
    dst_b[0] = b0; dst_b[1] = b1; dst_b[2] = b2; dst_b[3] = b3;
}

}  // namespace rtfhe
