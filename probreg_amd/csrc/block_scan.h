// Workgroup scans of the order-preserving compactions: global_reg.hip (the valid hypotheses) and voxel.hip (the run heads)
// count per tile, scan the tile counts with one workgroup and write in order.
#pragma once
#include <hip/hip_runtime.h>

namespace prg {

// inclusive scan of one int per lane over a workgroup of N lanes
template <int N>
__device__ __forceinline__ void scan_inclusive(int* cnt) {
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const int v = (int)threadIdx.x >= off ? cnt[threadIdx.x - off] : 0;
        __syncthreads();
        cnt[threadIdx.x] += v;
        __syncthreads();
    }
}

// Exclusive scan of ntiles counts by one workgroup of N lanes (cnt: N ints of LDS): a lane adds a run of consecutive tiles, the
// run sums are scanned, every tile gets its start; *total = the sum of all counts.
template <int N>
__device__ __forceinline__ void tile_scan(const int* __restrict__ tile_count, int ntiles, int* __restrict__ tile_start,
                                          int* __restrict__ total, int* cnt) {
    const int per = (ntiles + N - 1) / N;
    const int b = (int)threadIdx.x * per < ntiles ? (int)threadIdx.x * per : ntiles;
    const int e = b + per < ntiles ? b + per : ntiles;
    int c = 0;
    for (int t = b; t < e; ++t) c += tile_count[t];
    cnt[threadIdx.x] = c;
    scan_inclusive<N>(cnt);
    int pos = cnt[threadIdx.x] - c;
    for (int t = b; t < e; ++t) {
        tile_start[t] = pos;
        pos += tile_count[t];
    }
    if (threadIdx.x == N - 1) *total = cnt[threadIdx.x];
}

}  // namespace prg
