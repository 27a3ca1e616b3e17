// rtfhe_kernels_tlwe_seeded.hpp -- k_tlwe_seeded_expand: a seeded lvl0 object (public seed, first row, one b word per row) into rows of
// n + 1 words, a[0 .. n) then b, in one launch (include/rtfhe.h, "seeded lvl0 ciphertexts"; the CPU form and oracle: rtfhe_tlwe_seeded_expand in
// rtfhe_seeded.cpp).  A lane owns one ChaCha20 block (row r, block c) of the rows * ceil(n / 16) there are, but does not store it itself: n is
// no multiple of 16 and a row starts at any word, so no 16-byte store can be assumed, and 16 dword stores per lane would touch 64 separate 4-byte
// pieces each.  The wave's 64 blocks pass through a wave-private LDS image instead (17-word pitch: the 32 lanes of a ds_write_b32 group land
// on 32 banks), and in each of the 16 store instructions lane L writes word 64 j + L of the image: consecutive lanes, consecutive words of a row, a
// gap only where the wave's blocks pass a row's end.  The words of a row's last block at columns >= n are dropped; b[r] goes to column n from the
// lane that owns that block.  Integer only, static LDS, nothing allocated.  The seed rides in the kernel arguments: a stream capture bakes it in.
#pragma once

#include <hip/hip_runtime.h>

#include "rtfhe_chacha.hpp"
#include "rtfhe_device.hpp"

namespace rtfhe {

struct TlweSeededArgs {
    uint32_t seed[8];
    uint64_t first_row;
    const uint32_t* b;      // [rows]
    uint32_t* out;          // [rows][stride], columns 0 .. n written
    uint32_t blocks;        // rows * nb, below 2^31 (rtfhe_tlwe_seeded_plan)
    uint32_t n;             // 1 .. 767
    uint32_t nb;            // ceil(n / 16)
    uint32_t stride;        // words between rows, >= n + 1
};

constexpr int TLWE_SEEDED_THREADS = 256;
constexpr int TLWE_SEEDED_PITCH = 17;        // words per block in the LDS image

__global__ __launch_bounds__(TLWE_SEEDED_THREADS) void k_tlwe_seeded_expand(TlweSeededArgs a) {
    __shared__ uint32_t image[TLWE_SEEDED_THREADS * TLWE_SEEDED_PITCH];
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t* mine = image + (threadIdx.x - lane) * TLWE_SEEDED_PITCH;      // this wave's 64 blocks
    const uint32_t t = blockIdx.x * TLWE_SEEDED_THREADS + threadIdx.x;
    // (a lane past the last block owns nothing: its column is past every row's end, so the words read for it below are never stored)
    uint32_t r = 0, c = a.nb;
    if (t < a.blocks) {
        r = t / a.nb; c = t - r * a.nb;
        uint32_t ks[16];
        chacha_block(a.seed, (uint64_t)c, a.first_row + (uint64_t)r, ks);
#pragma unroll
        for (int i = 0; i < 16; i++) mine[lane * TLWE_SEEDED_PITCH + i] = ks[i];
        if (c == a.nb - 1) a.out[(size_t)r * a.stride + a.n] = a.b[r];
    }
    wave_lds_sync();
    const uint32_t i = lane & 15u;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int k = 4 * j + (int)(lane >> 4);      // the block of the wave that word 64 j + lane belongs to
        const uint32_t rk = (uint32_t)__shfl((int)r, k), col = 16u * (uint32_t)__shfl((int)c, k) + i;
        const uint32_t w = mine[k * TLWE_SEEDED_PITCH + i];
        if (col < a.n) a.out[(size_t)rk * a.stride + col] = w;
    }
}

}  // namespace rtfhe
