// rtfhe_kernels_lutc.hpp -- the two memory-bound steps around the many-LUT bootstrap of a LUT circuit wave (include/rtfhe.h:
// rtfhe_lut_circuit_create).  k_lut_gather writes every node's weighted sum of wires into the circuit's own [count][n+1] buffer (the input
// of the many-LUT PBS), k_lut_scatter copies the key-switched outputs [count][n_out][n+1] back into their wires.  One wave per row, 16-byte
// words when the row width allows (VEC: n+1 a multiple of 4 and the wire table 16-byte aligned).  Indices were checked on the host before
// the circuit was recorded; a row whose index is out of range is still never dereferenced (a gathered slot adds nothing, a scattered row is
// not stored).  Instantiated in rtfhe_circuit.hip.
#pragma once

#include "rtfhe_kernels.hpp"

namespace rtfhe {

constexpr int LUTC_WAVES = 4;     // rows per workgroup of both kernels, one wave each

struct LutGatherArgs {
    const uint32_t* wires;        // [num_wires][n1]
    uint32_t* out;                // [count][n1]
    const int32_t* in_idx;        // [count][F] wire indices, -1 = unused slot
    const int32_t* weights;       // [count][F]
    const uint32_t* cst;          // [count]: added to word n (b) only
    int32_t count, n1, num_wires;
};

struct LutScatterArgs {
    uint32_t* src;                // [rows][n1]: left zero (the next key switch adds into it)
    uint32_t* wires;              // [num_wires][n1]
    const int32_t* out_idx;       // [rows]
    int32_t rows, n1, num_wires;
};

// out[g] = sum_k weights[g][k] * wires[in_idx[g][k]] (wrapping u32, every word), then out[g][n] += cst[g]
template <int F, bool VEC>
__global__ __launch_bounds__(64 * LUTC_WAVES) void k_lut_gather(LutGatherArgs a) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * LUTC_WAVES + (threadIdx.x >> 6);
    if (g >= a.count) return;
    const uint32_t* src[F];
    uint32_t w[F];
#pragma unroll
    for (int k = 0; k < F; k++) {
        const int i = a.in_idx[(size_t)g * F + k];
        const bool used = (unsigned)i < (unsigned)a.num_wires;
        src[k] = a.wires + (size_t)(used ? i : 0) * a.n1;
        w[k] = used ? (uint32_t)a.weights[(size_t)g * F + k] : 0u;
    }
    const uint32_t cst = a.cst[g];
    uint32_t* dst = a.out + (size_t)g * a.n1;
    if constexpr (VEC) {
        const int q = a.n1 >> 2;
        for (int c = lane; c < q; c += 64) {
            uint4 t = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int k = 0; k < F; k++) {
                if (!w[k]) continue;      // unused slot (or weight 0): no load
                const uint4 v = reinterpret_cast<const uint4*>(src[k])[c];
                t.x += w[k] * v.x; t.y += w[k] * v.y; t.z += w[k] * v.z; t.w += w[k] * v.w;
            }
            if (c == q - 1) t.w += cst;
            reinterpret_cast<uint4*>(dst)[c] = t;
        }
    } else {
        for (int c = lane; c < a.n1; c += 64) {
            uint32_t t = 0u;
#pragma unroll
            for (int k = 0; k < F; k++)
                if (w[k]) t += w[k] * src[k][c];
            if (c == a.n1 - 1) t += cst;
            dst[c] = t;
        }
    }
}

// wires[out_idx[r]] = src[r], then src[r] = 0: the batch key switch of the next wave (or replay) adds its K-slices into a zero buffer without a
// memset in the graph
template <bool VEC>
__global__ __launch_bounds__(64 * LUTC_WAVES) void k_lut_scatter(LutScatterArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * LUTC_WAVES + (threadIdx.x >> 6);
    if (r >= a.rows) return;
    const int o = a.out_idx[r];
    const bool ok = (unsigned)o < (unsigned)a.num_wires;
    uint32_t* s = a.src + (size_t)r * a.n1;
    uint32_t* d = a.wires + (size_t)(ok ? o : 0) * a.n1;
    if constexpr (VEC) {
        const int q = a.n1 >> 2;
        for (int c = lane; c < q; c += 64) {
            const uint4 v = reinterpret_cast<const uint4*>(s)[c];
            if (ok) reinterpret_cast<uint4*>(d)[c] = v;
            reinterpret_cast<uint4*>(s)[c] = make_uint4(0u, 0u, 0u, 0u);
        }
    } else {
        for (int c = lane; c < a.n1; c += 64) {
            const uint32_t v = s[c];
            if (ok) d[c] = v;
            s[c] = 0u;
        }
    }
}

}  // namespace rtfhe
