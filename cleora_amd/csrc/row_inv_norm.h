// 1 / max(||x_r||, 1e-10) per row: the pass that knn.hip and kmeans.hip both start with.  Internal linkage: every translation unit that
// includes this gets its own copy of the kernel.
#pragma once

#include "common.h"

namespace cleora {
namespace {

__device__ __forceinline__ float wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inv[r] = 1 / max(||x_r||, 1e-10) for r < n, 0 up to n_pad (whole candidate tiles)
__global__ __launch_bounds__(256) void knn_inv_norm_kernel(const float *__restrict__ x, uint64_t ldx, uint64_t n, uint64_t n_pad,
                                                           uint32_t d, float *__restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * 4;
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n_pad; row += waves) {
        float sq = 0.f;
        if (row < n) {
            const float *xr = x + row * ldx;
            for (uint32_t c = lane; c < d; c += 64) sq += xr[c] * xr[c];
        }
        sq = wsum(sq);
        if (lane == 0) inv[row] = row < n ? 1.0f / fmaxf(sqrtf(sq), 1e-10f) : 0.0f;
    }
}

inline void launch_row_inv_norm(const float *x, uint64_t ldx, uint64_t n, uint64_t n_pad, uint32_t d, float *inv, hipStream_t stream) {
    const unsigned grid = (unsigned)((n_pad + 3) / 4 < 4096 ? (n_pad + 3) / 4 : 4096);
    hipLaunchKernelGGL(knn_inv_norm_kernel, dim3(grid), dim3(256), 0, stream, x, ldx, n, n_pad, d, inv);
}

}  // namespace
}  // namespace cleora
