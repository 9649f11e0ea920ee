// Device-side helpers shared by the translation units of libprobreg_hip.so.
#pragma once
#include <hip/hip_runtime.h>

// sum over the 64 lanes of a wave; lane 0 holds the total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
