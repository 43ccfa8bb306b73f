// The library's sums of one double per thread, each in ONE fixed order of additions: results that must not change by a bit between
// kernels, launches or releases add up through these and nowhere else.  (Reductions that carry several values through one tree keep
// their own loops: their interleaving is part of how they are scheduled.)
#pragma once
#include <hip/hip_runtime.h>

namespace {

// lane 0 <- the 64 lanes' values by the halving tree: lane i += lane i + 32, then + 16, 8, 4, 2, 1.  Valid in lane 0 only.
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// thread 0 <- the workgroup's values (any block of up to 1024 threads, a multiple of 64; sw: one double per wave in LDS): wave_sum
// per wave, then the waves' sums IN TURN, ((0.0 + w0) + w1) + w2 ...  Valid in thread 0 only; every thread of the block calls it.
__device__ __forceinline__ double block_sum(double s, double *sw) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sw[w];
    return t;
}

// the same for the 256-thread kernels, whose four waves are added in pairs: (w0 + w1) + (w2 + w3).  Valid in thread 0 only.
__device__ __forceinline__ double block_sum4(double s, double *sw) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    return threadIdx.x == 0 ? (sw[0] + sw[1]) + (sw[2] + sw[3]) : 0.0;
}

}  // namespace
