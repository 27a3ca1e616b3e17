// rtfhe_chacha.hpp -- the ChaCha20 block function (RFC 8439 2.3), once, for the host generators (rtfhe_sampling.hpp), the seeded ciphertexts'
// host unit (rtfhe_seeded.cpp) and their kernel (rtfhe_kernels_seeded.hpp).  State words 12-13 hold a 64-bit block counter and words 14-15 a
// 64-bit stream id: the RFC's keystream with a 32-bit counter and the nonce words (counter hi, stream lo, stream hi).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTFHE_HOST_DEVICE __host__ __device__
#else
#define RTFHE_HOST_DEVICE
#endif

namespace rtfhe {

RTFHE_HOST_DEVICE inline uint32_t chacha_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

#define RTFHE_CHACHA_QR(a, b, c, d)                                                          \
    a += b; d = chacha_rotl(d ^ a, 16); c += d; b = chacha_rotl(b ^ c, 12);                  \
    a += b; d = chacha_rotl(d ^ a, 8);  c += d; b = chacha_rotl(b ^ c, 7);

// out = the 16 keystream words of block `counter` of stream `stream` under `key`
RTFHE_HOST_DEVICE inline void chacha_block(const uint32_t key[8], uint64_t counter, uint64_t stream, uint32_t out[16]) {
    const uint32_t i0 = 0x61707865u, i1 = 0x3320646eu, i2 = 0x79622d32u, i3 = 0x6b206574u;
    const uint32_t i4 = key[0], i5 = key[1], i6 = key[2], i7 = key[3], i8 = key[4], i9 = key[5], i10 = key[6], i11 = key[7];
    const uint32_t i12 = (uint32_t)counter, i13 = (uint32_t)(counter >> 32), i14 = (uint32_t)stream, i15 = (uint32_t)(stream >> 32);
    uint32_t x0 = i0, x1 = i1, x2 = i2, x3 = i3, x4 = i4, x5 = i5, x6 = i6, x7 = i7, x8 = i8, x9 = i9, x10 = i10, x11 = i11, x12 = i12, x13 = i13,
             x14 = i14, x15 = i15;
    for (int r = 0; r < 10; r++) {
        RTFHE_CHACHA_QR(x0, x4, x8, x12) RTFHE_CHACHA_QR(x1, x5, x9, x13) RTFHE_CHACHA_QR(x2, x6, x10, x14) RTFHE_CHACHA_QR(x3, x7, x11, x15)
        RTFHE_CHACHA_QR(x0, x5, x10, x15) RTFHE_CHACHA_QR(x1, x6, x11, x12) RTFHE_CHACHA_QR(x2, x7, x8, x13) RTFHE_CHACHA_QR(x3, x4, x9, x14)
    }
    out[0] = x0 + i0; out[1] = x1 + i1; out[2] = x2 + i2; out[3] = x3 + i3; out[4] = x4 + i4; out[5] = x5 + i5; out[6] = x6 + i6; out[7] = x7 + i7;
    out[8] = x8 + i8; out[9] = x9 + i9; out[10] = x10 + i10; out[11] = x11 + i11; out[12] = x12 + i12; out[13] = x13 + i13; out[14] = x14 + i14;
    out[15] = x15 + i15;
}

#undef RTFHE_CHACHA_QR

}  // namespace rtfhe
