// The buffers of the CPD plan that are sized together (cpd_plan.h): the source group, the target group and the arrays of a sweep
// queue.  Each group is all-or-nothing: after every call either all of its buffers have the sizes of ONE capacity, or all are
// empty and the capacity is 0 - a failed allocation never leaves a group whose extents describe arrays that are not there.
// Host-compilable: depends on dev_buf.h and the HIP vector types only (tests/host/dev_buf_check.cpp runs it against a fake
// allocator).
#pragma once
#include <hip/hip_vector_types.h>

#include "dev_buf.h"

namespace prg {
constexpr int kGroup = 32;               // streamed points per cull group (8 scalar quad loads)
constexpr int kSuper = 256;              // quantum of a culled segment's length (8 groups)
constexpr int kMfmaWgPoints = 512;       // points a workgroup of the matrix-core sweeps owns and shifts to one origin
constexpr int kQueueChunkGroups = 512;   // streamed groups (of 32 points) one wave of the queue's build pass tests: 8 mask words

// Source cloud in its kernel layout (float4 per point: x, y, z, aux) and what is sized with it.
struct SourceBuffers {
    DevBuf<float4> src4;    // original source y_m            (aux = 0)
    DevBuf<float4> z4;      // transformed source z_m         (aux = 0), rewritten every E-step
    DevBuf<double> rowacc;  // fp64 per-row block [4][Mcap] (p1, px0, px1, px2), written by the moment kernel
    DevBuf<float> zmeta;    // [Mcap/32][8] per group of 32 transformed source points: lo.xyz, hi.xyz, -, -
    DevBuf<float4> rorig;   // [Mcap/512 + 4] origin of each 512-row block of the last matrix-core row pass
    DevBuf<float> zchunk;   // [Mcap/256][8] box of every 256-point chunk of the transformed source (per E-step)
    int64_t Mcap = 0;       // padded capacity (a multiple of 1024, + slack for segmenting)

    // exact sizes for `cap` points: kept when cap == Mcap, re-created as a whole otherwise (the contents are gone)
    hipError_t size_source(int64_t cap) {
        if (cap == Mcap) return hipSuccess;
        Mcap = 0;
        const hipError_t e = reset_group(src4, cap, z4, cap, rowacc, 4 * cap, zmeta, cap / kGroup * 8, rorig, cap / kMfmaWgPoints + 4,
                                         zchunk, cap / kSuper * 8);
        if (e == hipSuccess) Mcap = cap;
        return e;
    }
};

// Local target cloud and what is sized with it.
struct TargetBuffers {
    DevBuf<float4> tgt4;   // local target x_n               (aux = b_n = -log2(den_n + c))
    DevBuf<float> pt1;     // [Ncap] column sums of P
    DevBuf<float> tmeta;   // [Ncap/32][8] per group of 32 target points: lo.xyz, hi.xyz, max b_n, min b_n
    DevBuf<float> tchunk;  // [Ncap/256][8] box + largest b_n of every 256-point chunk of the target (per E-step)
    DevBuf<float4> corig;  // [Ncap/512 + 4] origin of each 512-column block of the last fused sweep
    DevBuf<float> colmin;  // [Ncap] min_m d^2 per column from the previous E-step (seed of the cull bound), followed by
                           // [Ncap/32] per-group maxima of it
    int64_t Ncap = 0;

    // as size_source; *recreated: the group is new (the owner zeroes colmin)
    hipError_t size_target(int64_t cap, bool* recreated) {
        *recreated = false;
        if (cap == Ncap) return hipSuccess;
        Ncap = 0;
        const hipError_t e = reset_group(tgt4, cap, pt1, cap, tmeta, cap / kGroup * 8, tchunk, cap / kSuper * 8, corig,
                                         cap / kMfmaWgPoints + 4, colmin, cap + cap / kGroup);
        if (e != hipSuccess) return e;
        Ncap = cap;
        *recreated = true;
        return hipSuccess;
    }
};

// Work queue of one sparse-regime sweep (cpd_sweeps_queue.hip): 16-bit need-masks per (owned block of 128 points, segment of 16
// streamed groups), the number of non-empty segments per block, and the units the persistent waves pop.
struct SweepQueue {
    DevBuf<unsigned long long> masks;  // [nblocks][nchunk][8] one bit per streamed group of 32: needed or not
    DevBuf<int2> chunk;                // [nblocks][nchunk] (first slot, units) of every chunk of 512 groups
    DevBuf<int2> units;                // [<= max units] (block, first group | count << 22), in append order
    DevBuf<int> ctrl;                  // counters, see k_queue_build
    DevBuf<unsigned> ucount;           // [units] (128 x 32) blocks each unit evaluated (prg_cpd_pair_counts)
    int64_t cap_blocks = 0, cap_units = 0;  // extents the arrays were created for
    int cap_chunk = 0;
    int64_t nblocks = 0;                    // ... and those of the last sweep built into them
    int nchunk = 0, cap_soft = 0;

    void release() {
        masks.release(); chunk.release(); units.release(); ctrl.release(); ucount.release();
        cap_blocks = cap_units = nblocks = 0;
        cap_chunk = nchunk = cap_soft = 0;
    }
    bool fits(int64_t blocks, int chunks, int64_t max_units) const {
        return blocks <= cap_blocks && chunks <= cap_chunk && max_units <= cap_units;
    }
    // grows only, and as a whole: larger in any one extent re-creates all five arrays at the new extents.  *recreated: the arrays
    // are new (the owner initialises ctrl)
    hipError_t size(int64_t blocks, int chunks, int64_t max_units, bool* recreated) {
        *recreated = false;
        if (fits(blocks, chunks, max_units)) return hipSuccess;
        const hipError_t e = reset_group(masks, blocks * chunks * (kQueueChunkGroups / 64), chunk, blocks * chunks, units, max_units,
                                         ctrl, 16, ucount, max_units);
        nblocks = 0;  // (the sweep built into the old arrays went with them)
        nchunk = cap_soft = 0;
        cap_blocks = e == hipSuccess ? blocks : 0;
        cap_chunk = e == hipSuccess ? chunks : 0;
        cap_units = e == hipSuccess ? max_units : 0;
        if (e != hipSuccess) return e;
        *recreated = true;
        return hipSuccess;
    }
};

}  // namespace prg
