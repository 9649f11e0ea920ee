// The CPD E-step (cpd_estep.hip) as the rest of the plan's code (cpd.hip) sees it: the layout of one E-step - segments, partial
// planes, which engines may run, buffer sizes - as a pure function of the plan, the driver, and the few pieces the moment
// kernels of the two files share.
#pragma once
#include <algorithm>

#include "cpd_plan.h"
#include "prg_device.h"

// Everything an E-step derives from the plan before its first launch.  A / col: the column pass (lanes own target columns, the
// transformed source is streamed); B / row: the row pass (lanes own source rows, the target is streamed).
struct EstepLayout {
    int ra, rb, RA, RB;        // points per lane as tuned (negative: scalar form) and their magnitudes
    bool use_cull;             // culled sweeps: both clouds spatially sorted, nothing pinned by prg_cpd_set_tuning
    int SA, segA, PA;          // column pass on the vector pipe: segments, their length, partial planes in HBM
    int SB, segB, PB;          // row pass
    bool mfma_possible;        // the dense regime may run on the matrix cores (decided per E-step on the device)
    int seg_col_fine, seg_row_fine;  // segments of a culling matrix-core launch (mfma_fine_segments; 0: the default grid)
    int PAm, PBm;              // most partial planes a matrix-core launch can write, however it is cut
    bool use_queue;            // sparse regime over the device-built work queue (cpd_sweeps_queue.hip)
    bool allow_fused;          // this E-step may run as the fused single sweep on the matrix cores
    bool allow_resid;          // ... as the residual-form single sweep on the vector pipe
    bool use_owner;            // ... which the column block's owner runs (cpd_sweeps_owner.hip)
    int PO;                    // ... over this many partial planes
    int64_t colpart_elems, rowpart_elems, wgcount_elems, mompart_elems;  // float2 / float / workgroups / doubles
};

namespace prg {
constexpr int kBlock = 256;
constexpr int kMomComp = 24;
inline dim3 grid1(int64_t n) { return dim3((unsigned)ceil_div(n, kBlock)); }

int estep_layout(const prg_cpd& h, EstepLayout* L);  // no HIP call, no allocation, no getenv
int estep_impl(prg_cpd* h, double w, hipEvent_t* ev);  // ev: null, or the six timing points of prg_cpd_estep_timed
double engine_col_bound(int64_t m, int64_t n_local);
double engine_row_bound(int64_t m, int64_t n_local, bool lean = true);
int ensure_engine_state(prg_cpd* h);  // (cpd.hip)

// [mom_blocks][24] block partials of the moment kernels, then [mom_blocks][2] partials of (sum pt1 |x|^2, sum pt1) (k_colfinal), then
// 64 doubles of scratch at the very end
inline int mom_blocks(const prg_cpd& h) { return (int)ceil_div(std::max(h.M, h.N), kBlock); }
inline int64_t mompart_elems(const prg_cpd& h) { return (int64_t)mom_blocks(h) * (kMomComp + 2) + 64; }
int ensure_mompart(prg_cpd* h);
// ... of the ALLOCATION (mompart grows and never shrinks: the end of the block a larger cloud pair left is the one place every
// reader and writer agrees on)
inline double* mom_scratch(const prg_cpd& h) { return h.mompart.p + (h.mompart.cap - 64); }
// out[off + c] = sum_b part[b][ncomp] (k_reduce_partials, one workgroup), on the plan's stream
void reduce_partials(prg_cpd* h, const double* part, int nblk, int ncomp, double* out, int off);

// fp64 moment reduction: per row, then per block -> mompart[nblk][24]
__device__ __forceinline__ void block_reduce_store(double (&a)[kMomComp], double* __restrict__ mompart) {
    __shared__ double sh[4][kMomComp];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < kMomComp; ++c) {
        const double s = wave_sum(a[c]);
        if (lane == 0) sh[wv][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < kMomComp)
        mompart[(int64_t)blockIdx.x * kMomComp + threadIdx.x] =
            sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

__device__ __forceinline__ void row_moment_terms(double (&a)[kMomComp], double p1, const double (&px)[3],
                                                 const double (&y)[3]) {
    a[0] = p1;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[1 + i] = px[i];
        a[4 + i] = p1 * y[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) a[7 + 3 * i + j] = px[i] * y[j];
    }
    a[16] = p1 * y[0] * y[0];
    a[17] = p1 * y[0] * y[1];
    a[18] = p1 * y[0] * y[2];
    a[19] = p1 * y[1] * y[1];
    a[20] = p1 * y[1] * y[2];
    a[21] = p1 * y[2] * y[2];
}
}  // namespace prg
