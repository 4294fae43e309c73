// Fixed-order sum of per-workgroup partial results - the second kernel of every "each workgroup keeps its accumulators, then
// the partials are added" reduction (conv1_bwd_kernel in trunk.hip, conv3x3_wrw_kernel in conv_wrw.hip): deterministic, no
// atomics, no zero-fill.
#pragma once
#include "hk_common.h"

namespace hk {

// part [nblk][nel] -> out0[e] for e < nsplit, out1[e - nsplit] for the rest (nsplit = nel: one output, out1 unused).
// 64 elements per workgroup of 64 Q threads, Q interleaved chains per element (eight loads in flight each), combined in order
template <int Q>
__global__ __launch_bounds__(64 * Q) void partial_sum_kernel(const float* __restrict__ part, int nblk, int nel, int nsplit,
                                                             float* __restrict__ out0, float* __restrict__ out1) {
    __shared__ float red[Q][64];
    const int l = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + l;
    float s = 0.f;
    if (e < nel) {
        int k = q;
        for (; k + 7 * Q < nblk; k += 8 * Q) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(long long)(k + Q * u) * nel + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; k < nblk; k += Q) s += part[(long long)k * nel + e];
    }
    red[q][l] = s;
    __syncthreads();
    if (q == 0 && e < nel) {
        float t = red[0][l];
        for (int k = 1; k < Q; ++k) t += red[k][l];
        if (e < nsplit) out0[e] = t;
        else out1[e - nsplit] = t;
    }
}

}  // namespace hk
