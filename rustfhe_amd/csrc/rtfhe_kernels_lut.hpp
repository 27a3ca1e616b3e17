// rtfhe_kernels_lut.hpp -- the one kernel of the table unit: the wrapping sum of TRLWEs (the leaves of a CMUX demultiplexer,
// rtfhe_kernels_demux_tree.hpp) into the rows of an encrypted table (include/rtfhe.h: rtfhe_lut_accumulate_dev).  A plain __global__, not a
// template: included by rtfhe_lut.hip alone, where it is instantiated.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace rtfhe {

struct TrlweAccumulateArgs {
    uint32_t* rows;            // the table's rows [first, first + n): [n][2][N]
    const uint32_t* src;       // [count][n][2][N]
    size_t words;              // n * 2N
    int32_t count;
};

// rows[w] += sum over g of src[g][w], wrapping: a thread per table word, plain vector loads and stores, no atomics (every word has one owner)
__global__ __launch_bounds__(256) void k_trlwe_accumulate(const TrlweAccumulateArgs a) {
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= a.words) return;
    uint32_t sum = a.rows[w];
    for (int g = 0; g < a.count; g++) sum += a.src[(size_t)g * a.words + w];
    a.rows[w] = sum;
}

}  // namespace rtfhe
