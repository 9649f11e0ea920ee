// The CPD E-step for MI355X (gfx950): its layout, the per-E-step engine decision, the launches, and the kernels that merge the
// sweeps' partial results into b_n / pt1_n and the fp64 moments.  (The pair sweeps themselves: cpd_sweeps_*.hip; plan lifecycle,
// uploads, the M-step and the C ABI: cpd.hip.)
//
// Reference behaviour (neka-nat/probreg v0.3.7):  E-step  probreg/cpd.py:71-88,  transforms  probreg/transformation.py:49-50, 77-78
//
// Design: the M x N responsibility matrix is never stored.
//   k_colpass  lane owns R target columns, streams a segment of the transformed source through
//              SGPRs (scalar loads, wave-uniform), keeps an online (min d^2, sum exp2) pair.
//   k_colfinal merges the segment partials in fp64 -> b_n = -log2(den_n + c), pt1_n.
//   k_rowpass  lane owns R source rows, streams a segment of (x_n, b_n) through SGPRs and
//              accumulates p1, u = sum P (x - z), e = sum P |x - z|^2 (residual form, fp32).
//   k_row_moments  sums the segment partials per row in fp64, rebuilds px = u + p1 z and the
//              23 fp64 moments the rigid / affine M-step needs (the RCCL all-reduce payload).
// A RIGID iteration (prg_cpd_iterate, prg_cpd_set_moments_only) runs ONE sweep instead of two: the column
// pass carries per-column sums of the source side as well - on the matrix cores relative to a block origin (k_colpass_mfma<FUSED> ->
// k_colfinal_fused), on the vector pipe as residuals against the column's own x_n (k_colpass_cull<true> / k_colpass_queue<true> ->
// k_colfinal_resid) - and k_fused_final maps the z-side sums back to the source's frame: no row pass, no per-point block.
//
// The driver, estep_impl at the end of this file, is a sequence of steps: layout (estep_layout: a pure function of the plan) ->
// buffers -> transform -> engine decision (decide_engines) -> column pass -> merge tail (one sweep or two).
#include <math.h>

#include <algorithm>
#include <cmath>

#include "cpd_estep.h"
#include "cpd_sweeps.h"

namespace {
using prg::block_reduce_store;
using prg::grid1;
using prg::kBlock;
using prg::kMomComp;
using prg::row_moment_terms;

constexpr double kLog2e = 1.4426950408889634;

// out[off + c] = sum_b part[b][ncomp] ; one block of 1024 threads (32 slices x 32 components), ncomp <= 32
constexpr int kRedBlock = 1024;
__global__ __launch_bounds__(kRedBlock) void k_reduce_partials(const double* __restrict__ part, int nblk, int ncomp,
                                                               double* __restrict__ out, int off) {
    __shared__ double sh[32][33];
    const int c = threadIdx.x & 31, slice = threadIdx.x >> 5;
    double s = 0.0;
    if (c < ncomp)
        for (int b = slice; b < nblk; b += 32) s += part[(int64_t)b * ncomp + c];
    sh[slice][c] = s;
    __syncthreads();
    if (threadIdx.x < ncomp) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) t += sh[k][threadIdx.x];
        out[off + threadIdx.x] = t;
    }
}

// half-wave (32-lane) reductions: a cull group is 32 consecutive points = one half of a wave
__device__ __forceinline__ float half_min(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float half_max(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Writes the boxes of the 8 groups of 32 points this workgroup holds (one point per thread): lo.xyz, hi.xyz, max aux,
// min aux.  write_boxes == false: only the aux range is refreshed (the boxes of a static cloud were written at upload).
__device__ __forceinline__ void block_group_meta(float x, float y, float z, float wmax_in, float wmin_in,
                                                 bool write_boxes, float* __restrict__ gmeta, float* box_out = nullptr,
                                                 bool real = true) {
    float v[8];
    // (real == false: a pad; a group of real points and pads gets the box of its real points, an all-pad group the pads' own)
    v[0] = half_min(real ? x : INFINITY); v[1] = half_min(real ? y : INFINITY); v[2] = half_min(real ? z : INFINITY);
    v[3] = half_max(real ? x : -INFINITY); v[4] = half_max(real ? y : -INFINITY); v[5] = half_max(real ? z : -INFINITY);
    if (v[0] == INFINITY) {
        v[0] = v[3] = x; v[1] = v[4] = y; v[2] = v[5] = z;
    }
    v[6] = half_max(wmax_in);
    v[7] = half_min(wmin_in);
    if ((threadIdx.x & 31) == 0) {
        float* o = gmeta + ((int64_t)blockIdx.x * 8 + (threadIdx.x >> 5)) * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (write_boxes || c >= 6) o[c] = v[c];
    }
    if (box_out)
#pragma unroll
        for (int c = 0; c < 6; ++c) box_out[c] = v[c];
}

// z = scale * L y + t in fp64, rounded once to fp32 (transformation.py:49-50 / 77-78).  The same kernel measures
// how far the source moved since the previous E-step (cull bound of k_colpass_cull) and writes the group
// boxes of the transformed cloud.  grid = ceil(M / 256), one point per thread (pad-only blocks keep their static boxes).
__global__ __launch_bounds__(kBlock) void k_transform_linear(const float4* __restrict__ src4, float4* __restrict__ z4,
                                                             int64_t m, const double* __restrict__ params,
                                                             unsigned* __restrict__ motion, int slot,
                                                             float* __restrict__ gmeta,
                                                             const float* __restrict__ srcw,
                                                             const double* __restrict__ disp,
                                                             float* __restrict__ cmeta) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    float moved = 0.f;
    float4 o;
    if (i < m) {
        const double s = params[12];
        float4 y = src4[i];
        double yx = y.x, yy = y.y, yz = y.z;
        if (disp) {  // BCPD: z = s R (y + v_hat) + t  (CombinedTransformation, transformation.py)
            yx += disp[i * 3];
            yy += disp[i * 3 + 1];
            yz += disp[i * 3 + 2];
        }
        o.x = (float)(s * (params[0] * yx + params[1] * yy + params[2] * yz) + params[9]);
        o.y = (float)(s * (params[3] * yx + params[4] * yy + params[5] * yz) + params[10]);
        o.z = (float)(s * (params[6] * yx + params[7] * yy + params[8] * yz) + params[11]);
        // weight a_m as an extra squared distance: a_m exp(-d2 / 2 sigma2) = exp(-(d2 + q_m) / 2 sigma2)
        o.w = srcw ? (float)(-2.0 * params[13] * (double)srcw[i]) : 0.f;
        const float4 old = z4[i];
        const float dx = o.x - old.x, dy = o.y - old.y, dz = o.z - old.z;
        moved = sqrtf(dx * dx + dy * dy + dz * dz) * 1.000001f;
    } else {
        o.x = o.y = o.z = prg::kSrcPad;
        o.w = 0.f;
    }
    z4[i] = o;
    // non-negative floats order like their bit patterns: one atomicMax per wave into this E-step's slot; the other
    // slot (next E-step's) is cleared here - nobody touches it until the next launch of this kernel
    // (one atomic per workgroup: ~1600 same-address atomics from every wave cost more than the rest of the kernel)
    __shared__ float wave_moved[kBlock / 64];
    __shared__ float half_box[kBlock / 32][6];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) moved = fmaxf(moved, __shfl_xor(moved, off, 64));
    if ((threadIdx.x & 63) == 0) wave_moved[threadIdx.x >> 6] = moved;
    // the boxes of the block's 8 groups of 32 points, and - the block IS one 256-point chunk of the stream - their union: the box
    // of the chunk (zchunk; level 1 of the owner sweep's hierarchy, cpd_sweeps_owner.hip, in every regime)
    float gb[6];
    block_group_meta(o.x, o.y, o.z, 0.f, 0.f, true, gmeta, gb, i < m);
    if ((threadIdx.x & 31) == 0)
#pragma unroll
        for (int c = 0; c < 6; ++c) half_box[threadIdx.x >> 5][c] = gb[c];
    __syncthreads();
    if (threadIdx.x == 0) {
        float mv = wave_moved[0];
#pragma unroll
        for (int k = 1; k < kBlock / 64; ++k) mv = fmaxf(mv, wave_moved[k]);
        if (mv > 0.f) atomicMax(motion + slot, __float_as_uint(mv));
    }
    if (threadIdx.x < 6 && cmeta) {
        float v = half_box[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kBlock / 32; ++k) v = threadIdx.x < 3 ? fminf(v, half_box[k][threadIdx.x]) : fmaxf(v, half_box[k][threadIdx.x]);
        cmeta[(int64_t)blockIdx.x * 8 + threadIdx.x] = v;
    }
    if (i == 0) {
        motion[slot ^ 1] = 0u;
        motion[4 + slot] = 0u;  // k_colfinal of THIS E-step collects the largest column minimum here
    }
}

// (the two pair sweeps live in cpd_sweeps_packed.hip / cpd_sweeps_scalar.hip / cpd_sweeps_mfma.hip)

// Consumers of a sweep over the work queue (cpd_sweeps_queue.hip): the partial results of a block of 128 owned points sit
// in the slots of its units; chunk[b][c] = (first slot, units) for every chunk of 32 stream segments.  Walking the chunks
// and their units in order gives every block a fixed summation order, wherever the atomics placed the units.
struct QueueView {
    const int2* chunk;  // null: the sweep did not run over the queue
    int nchunk;
    int* ctrl;          // reset for the next E-step by the consumer's first thread
    int pop_start, cap_soft;
};
__device__ __forceinline__ void queue_reset(const QueueView& q) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int fine = q.ctrl[0] < q.cap_soft ? q.ctrl[0] : q.cap_soft;
        q.ctrl[8] = fine;                   // fine / coarse units of this sweep (prg_cpd_pair_counts)
        q.ctrl[9] = q.ctrl[7];
        q.ctrl[2] = q.ctrl[0];              // the next build sizes its units from this sweep's count ...
        q.ctrl[3] = q.ctrl[6];              // ... and unit size
        q.ctrl[0] = 0;                      // it appends from slot 0 ...
        q.ctrl[7] = 0;
        q.ctrl[1] = q.pop_start;            // ... and its waves take the first `pop_start` units without asking
    }
}

// Merge the S partial (min, sum) pairs of each column in fp64; apply cpd.py:78-82:
//   den == 0 -> eps32 (then the whole column of P is 0/eps = 0), den += c.
// Writes b_n = -log2(den_n) into tgt4[n].w so that P_mn = exp2(kk d2 + b_n), and pt1_n = den/(den+c).
__global__ __launch_bounds__(kBlock) void k_colfinal(float4* __restrict__ tgt4, const float2* __restrict__ colpart,
                                                     int nseg, int64_t ncap, int64_t n, float* __restrict__ pt1,
                                                     const double* __restrict__ params, double w, double m_over_n,
                                                     int dim, float* __restrict__ colmin, float* __restrict__ colmin_g,
                                                     float* __restrict__ gmeta, int seed_mode,
                                                     unsigned* __restrict__ stat, int slot, const QueueView qv,
                                                     double* __restrict__ xpart) {
    const int64_t i_own = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (qv.chunk) queue_reset(qv);
    float b = 0.f;  // pads keep b = 0
    float cmin = 0.f;  // pads do not widen the seed
    // Lanes past the end redo the last column and store nothing: the wave stays whole, which the queue consumer below
    // (entries handed round with readlane) relies on.
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    {
    const double sigma2 = params[13];
    const float kkf = (float)(-kLog2e / (2.0 * sigma2));
    // Online merge of the segment partials (dmin_s, sum_s), 8 in flight per lane.  sum_s is relative to the
    // exponent offset off_s = col_offset(kk, dmin_s) the column pass used (reproduced bit for bit), i.e. the true
    // segment sum is sum_s * 2^(-off_s).  The rescale factors are <= 1 and go through v_exp_f32 like the sweeps'
    // own (their 1-ulp error is far below the fp32 sums they multiply); the running sum is fp64.
    float gmin = INFINITY, goff = INFINITY;  // goff = smallest offset seen = offset of the column minimum
    double ssum = 0.0;
    if (seed_mode) {
        // matrix-core column pass: every segment's sum is relative to the SAME offset, known before the sweep
        // (prg::col_seed_offset from the previous E-step's minimum, still in colmin[i], and this E-step's motion)
        // (seed_mode 2: the first E-step's sweep ran without offsets)
        goff = seed_mode == 2 ? 0.f : prg::col_seed_offset(kkf, colmin[i], __uint_as_float(stat[slot]));
        for (int s0 = 0; s0 < nseg; ++s0) {
            const float2 p = colpart[(int64_t)s0 * ncap + i];
            gmin = fminf(gmin, p.x);
            ssum += (double)p.y;
        }
    } else if (qv.chunk) {
        // the slots of the column's block of 128, [unit][128] (min, sum) pairs, chunk by chunk, unit by unit: the wave's
        // 64 columns share the block, so lane c fetches chunk c's (first slot, units) entry once and the walk hands them
        // round with readlane; four units (four loads) are in flight per trip
        const int2* __restrict__ cb = qv.chunk + (i >> 7) * qv.nchunk;
        const int lane = threadIdx.x & 63;
        for (int c0 = 0; c0 < qv.nchunk; c0 += 64) {
            const int2 mine = c0 + lane < qv.nchunk ? cb[c0 + lane] : make_int2(0, 0);
            const int lim = qv.nchunk - c0 < 64 ? qv.nchunk - c0 : 64;
            int c = -1, left = 0, next = 0;
            auto next_slot = [&]() -> int {  // (wave-uniform)
                while (left == 0) {
                    if (++c >= lim) return -1;
                    next = __builtin_amdgcn_readlane(mine.x, c);
                    left = __builtin_amdgcn_readlane(mine.y, c);
                }
                --left;
                return next++;
            };
            for (;;) {
                int sl[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) sl[q] = next_slot();
                if (sl[0] < 0) break;
                float2 p[4];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    p[q] = sl[q] < 0 ? make_float2(INFINITY, 0.f) : colpart[(int64_t)sl[q] * 128 + (i & 127)];
                const float cm = fminf(fminf(p[0].x, p[1].x), fminf(p[2].x, p[3].x));
                if (cm < gmin) {
                    const float noff = prg::col_offset(kkf, cm);
                    ssum *= (double)__builtin_amdgcn_exp2f(noff - goff);
                    gmin = cm;
                    goff = noff;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (p[q].y != 0.f) ssum += (double)(p[q].y * __builtin_amdgcn_exp2f(goff - prg::col_offset(kkf, p[q].x)));
                if (sl[3] < 0) break;
            }
        }
    } else
    for (int s0 = 0; s0 < nseg; s0 += 8) {
        float2 p[8];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            p[k] = (s0 + k < nseg) ? colpart[(int64_t)(s0 + k) * ncap + i] : make_float2(INFINITY, 0.f);
        float cm = p[0].x;
#pragma unroll
        for (int k = 1; k < 8; ++k) cm = fminf(cm, p[k].x);
        if (cm < gmin) {
            const float noff = prg::col_offset(kkf, cm);
            ssum *= (double)__builtin_amdgcn_exp2f(noff - goff);  // first chunk: 0 * exp2(-inf) = 0
            gmin = cm;
            goff = noff;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)  // culled segments are empty (sum 0, min = inf or their seed bound)
            if (p[k].y != 0.f) ssum += (double)(p[k].y * __builtin_amdgcn_exp2f(goff - prg::col_offset(kkf, p[k].x)));
    }
    const double den = ssum * exp2(-(double)goff);  // underflows to 0 exactly where fp64 exp() does
    double c = 0.0;  // uniform (outlier) term of cpd.py:78-79; w == 0 is the common case and fp64 pow() is not free
    if (w > 0.0) c = pow(2.0 * M_PI * sigma2, dim * 0.5) * (w / (1.0 - w) * m_over_n);
    float p;
    if (den == 0.0) {
        b = -INFINITY;
        p = 0.f;
    } else {
        const double tot = den + c;
        b = (float)(-log2(tot));
        p = (float)(den / tot);
    }
    if (valid) {
        reinterpret_cast<float*>(tgt4 + i)[3] = b;
        pt1[i] = p;
        colmin[i] = gmin;  // min_m |x_n - z_m|^2 of this E-step: seed of the next column pass' cull bound
        cmin = gmin;
    } else {
        b = 0.f;
    }
    // (sum_n pt1_n |x_n|^2, sum_n pt1_n) of this workgroup's columns, for a row pass that does not carry the residual sums
    if (xpart) {
        const float4 xf = tgt4[i];
        const double ps = valid ? (double)p : 0.0;
        const double xs = ps * ((double)xf.x * xf.x + (double)xf.y * xf.y + (double)xf.z * xf.z);
        __shared__ double xsum[kBlock / 64][2];
        const double wx = wave_sum(xs), wp = wave_sum(ps);
        if ((threadIdx.x & 63) == 0) {
            xsum[threadIdx.x >> 6][0] = wx;
            xsum[threadIdx.x >> 6][1] = wp;
        }
        __syncthreads();
        if (threadIdx.x < 2) {
            double t = xsum[0][threadIdx.x];
#pragma unroll
            for (int k = 1; k < kBlock / 64; ++k) t += xsum[k][threadIdx.x];
            xpart[2 * (int64_t)blockIdx.x + threadIdx.x] = t;
        }
    }
    }
    // per group of 32 columns: the largest of these minima - what a wave of the next column pass needs for its seed
    {
        const float gm = half_max(cmin);
        if ((threadIdx.x & 31) == 0) colmin_g[(int64_t)blockIdx.x * (kBlock / 32) + (threadIdx.x >> 5)] = gm;
        // largest column minimum of the whole shard: the host's bracket check for the next matrix-core column pass
        __shared__ float wg_max[kBlock / 32];
        if ((threadIdx.x & 31) == 0) wg_max[threadIdx.x >> 5] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            float mx = wg_max[0];
#pragma unroll
            for (int k = 1; k < kBlock / 32; ++k) mx = fmaxf(mx, wg_max[k]);
            if (mx > 0.f) atomicMax(stat + 4 + slot, __float_as_uint(mx));  // (+inf orders above every finite value)
        }
    }
    // refresh the b_n range of this workgroup's 8 groups (their boxes are static)
    if (gmeta) block_group_meta(0.f, 0.f, 0.f, b, b, false, gmeta);
}

// ---------------------------------------------------------------------------------------------
// Fused single sweep of a rigid EM iteration (cpd_sweeps_mfma.hip, k_colpass_mfma<FUSED>): per column n the planes hold
// (min d^2, A, Bx, By, Bz, E) with A = sum_m K, B = sum_m K (z_m - o), E = sum_m K |z_m - o|^2, K = exp2(kk d^2 + L_n), o the
// origin of the column's 512-block.  This kernel is k_colfinal (den_n, pt1_n, b_n, the seeds of the next column pass) AND the
// moment kernel: with q_n = pt1_n / A_n the column contributes
//   [0] pt1   [1..3] pt1 x   [4..6] pz = q B + pt1 o   [7..15] x pz^T   [16] q (E + 2 o.B) + pt1 |o|^2   [22] pt1 |x|^2
// (block partials in mompart; k_fused_final sums them and maps the z-side sums back to the source's own frame).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_colfinal_fused(float4* __restrict__ tgt4, const float* __restrict__ fpart, int nseg,
                                                           int64_t ncap, int64_t n, float* __restrict__ pt1,
                                                           const double* __restrict__ params, double w, double m_over_n, int dim,
                                                           float* __restrict__ colmin, float* __restrict__ colmin_g,
                                                           float* __restrict__ gmeta, int seed_mode, unsigned* __restrict__ stat,
                                                           int slot, const float4* __restrict__ corig,
                                                           double* __restrict__ mompart) {
    const int64_t i_own = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;
    const double sigma2 = params[13];
    const float kkf = (float)(-kLog2e / (2.0 * sigma2));
    // every plane's sums are relative to the SAME exponent offset, known before the sweep (as in k_colfinal's seed mode)
    const float goff = seed_mode == 2 ? 0.f : prg::col_seed_offset(kkf, colmin[i], __uint_as_float(stat[slot]));
    float gmin = INFINITY;
    double A = 0.0, B[3] = {0.0, 0.0, 0.0}, E = 0.0;
    for (int s0 = 0; s0 < nseg; ++s0) {
        const float* __restrict__ q = fpart + (int64_t)s0 * 6 * ncap + i;
        gmin = fminf(gmin, q[0]);
        A += (double)q[ncap];
        B[0] += (double)q[2 * ncap];
        B[1] += (double)q[3 * ncap];
        B[2] += (double)q[4 * ncap];
        E += (double)q[5 * ncap];
    }
    const double den = A * exp2(-(double)goff);  // underflows to 0 exactly where fp64 exp() does
    double c = 0.0;
    if (w > 0.0) c = pow(2.0 * M_PI * sigma2, dim * 0.5) * (w / (1.0 - w) * m_over_n);
    float b, p;
    double pd = 0.0, qn = 0.0;
    if (den == 0.0) {  // cpd.py:81: den = eps32, the column of P is all zero
        b = -INFINITY;
        p = 0.f;
    } else {
        const double tot = den + c;
        b = (float)(-log2(tot));
        pd = den / tot;
        p = (float)pd;
        qn = pd / A;
    }
    float cmin = 0.f;
    double a[kMomComp];
#pragma unroll
    for (int k = 0; k < kMomComp; ++k) a[k] = 0.0;
    if (valid) {
        reinterpret_cast<float*>(tgt4 + i)[3] = b;
        pt1[i] = p;
        colmin[i] = gmin;
        cmin = gmin;
        const float4 xf = tgt4[i], of = corig[i / prg::kMfmaWgPoints];
        const double x[3] = {xf.x, xf.y, xf.z}, o[3] = {of.x, of.y, of.z};
        double pz[3], ob = 0.0, oo = 0.0, xx = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pz[k] = qn * B[k] + pd * o[k];
            ob += o[k] * B[k];
            oo += o[k] * o[k];
            xx += x[k] * x[k];
        }
        a[0] = pd;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[1 + r] = pd * x[r];
            a[4 + r] = pz[r];
#pragma unroll
            for (int k = 0; k < 3; ++k) a[7 + 3 * r + k] = x[r] * pz[k];
        }
        a[16] = qn * (E + 2.0 * ob) + pd * oo;
        a[22] = pd * xx;
    } else {
        b = 0.f;
    }
    block_reduce_store(a, mompart);
    {  // per group of 32 columns the largest of the minima, and the shard's largest (exactly as k_colfinal)
        const float gm = half_max(cmin);
        if ((threadIdx.x & 31) == 0) colmin_g[(int64_t)blockIdx.x * (kBlock / 32) + (threadIdx.x >> 5)] = gm;
        __shared__ float wg_max[kBlock / 32];
        if ((threadIdx.x & 31) == 0) wg_max[threadIdx.x >> 5] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            float mx = wg_max[0];
#pragma unroll
            for (int k = 1; k < kBlock / 32; ++k) mx = fmaxf(mx, wg_max[k]);
            if (mx > 0.f) atomicMax(stat + 4 + slot, __float_as_uint(mx));
        }
    }
    if (gmeta) block_group_meta(0.f, 0.f, 0.f, b, b, false, gmeta);
}

// ---------------------------------------------------------------------------------------------
// Residual-form single sweep of a rigid EM iteration on the vector pipe (k_colpass_cull<true> / k_colpass_queue<true>,
// DESIGN.md 3.1f): per column n the partials hold (min d^2, A, Ux, Uy, Uz, R) with A = sum_m K, U = sum_m K (x_n - z_m),
// R = sum_m K |x_n - z_m|^2, K = exp2(kk d^2 + off), off the offset of the partial's OWN minimum (prg::col_offset).  This
// kernel merges them online in fp64 (k_colfinal's merge with five channels), applies cpd.py:78-82 (den == 0 -> eps32, + c),
// writes b_n / pt1_n / the next column pass' seeds AND the column's share of the rigid M-step's moments - k_colfinal_fused's
// terms with the column's own x_n as the origin:  sum_m K z = x A - U,  sum_m K |z|^2 = |x|^2 A - 2 x.U + R:
//   [0] pt1   [1..3] pt1 x   [4..6] pz = pt1 x - q U   [7..15] x pz^T   [16] pt1 |x|^2 + q (R - 2 x.U)   [22] pt1 |x|^2,
// q = pt1 / A.  The sums are residuals against the CURRENT transformation (small where P is not), so sigma2 keeps the accuracy of
// the row pass' residual form at any amplification mean|x|^2 / (sigma2 D) - unlike the matrix-core fused sweep, whose
// origin is a 512-column block's.  k_fused_final maps the z-side sums back to the source's frame.
// QUEUE: the partials are the slots of the block's units, [unit][6][128], walked chunk by chunk, unit by unit (fixed order);
// otherwise planes [plane][6][ncap] with one touched flag per (128-column block, plane) behind them.
// ---------------------------------------------------------------------------------------------
template <bool QUEUE>
__global__ __launch_bounds__(kBlock) void k_colfinal_resid(float4* __restrict__ tgt4, const float* __restrict__ fpart, int nseg,
                                                           int64_t ncap, int64_t n, float* __restrict__ pt1,
                                                           const double* __restrict__ params, double w, double m_over_n, int dim,
                                                           float* __restrict__ colmin, float* __restrict__ colmin_g,
                                                           float* __restrict__ gmeta, unsigned* __restrict__ stat, int slot,
                                                           const unsigned char* __restrict__ colflag, const QueueView qv,
                                                           double* __restrict__ mompart, int flag_shift) {
    const int64_t i_own = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (QUEUE) queue_reset(qv);
    const bool valid = i_own < n;
    const int64_t i = valid ? i_own : n - 1;  // lanes past the end redo the last column and store nothing: the wave stays whole
    const int lane = threadIdx.x & 63;
    const double sigma2 = params[13];
    const float kkf = (float)(-kLog2e / (2.0 * sigma2));
    float gmin = INFINITY, goff = INFINITY;
    double A = 0.0, U[3] = {0.0, 0.0, 0.0}, R = 0.0;
    auto merge = [&](float pm, float a, float u0, float u1, float u2, float r) {
        if (pm < gmin) {
            const float noff = prg::col_offset(kkf, pm);
            const double f = (double)__builtin_amdgcn_exp2f(noff - goff);  // first partial: 0 * exp2(-inf) = 0
            A *= f; U[0] *= f; U[1] *= f; U[2] *= f; R *= f;
            gmin = pm;
            goff = noff;
        }
        if (a != 0.f) {
            const float f = __builtin_amdgcn_exp2f(goff - prg::col_offset(kkf, pm));
            A += (double)(a * f);
            U[0] += (double)(u0 * f);
            U[1] += (double)(u1 * f);
            U[2] += (double)(u2 * f);
            R += (double)(r * f);
        }
    };
    if (QUEUE) {
        const int2* __restrict__ cb = qv.chunk + (i >> 7) * qv.nchunk;
        for (int c0 = 0; c0 < qv.nchunk; c0 += 64) {
            const int2 mine = c0 + lane < qv.nchunk ? cb[c0 + lane] : make_int2(0, 0);
            const int lim = qv.nchunk - c0 < 64 ? qv.nchunk - c0 : 64;
            int c = -1, left = 0, next = 0;
            auto next_slot = [&]() -> int {  // (wave-uniform)
                while (left == 0) {
                    if (++c >= lim) return -1;
                    next = __builtin_amdgcn_readlane(mine.x, c);
                    left = __builtin_amdgcn_readlane(mine.y, c);
                }
                --left;
                return next++;
            };
            for (;;) {  // four units (24 loads) in flight per trip, merged in order
                int sl[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) sl[q] = next_slot();
                if (sl[0] < 0) break;
                float v[4][6];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float* __restrict__ o = fpart + (int64_t)(sl[q] < 0 ? sl[0] : sl[q]) * 768 + (i & 127);
#pragma unroll
                    for (int k = 0; k < 6; ++k) v[q][k] = o[128 * k];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (sl[q] >= 0) merge(v[q][0], v[q][1], v[q][2], v[q][3], v[q][4], v[q][5]);
                if (sl[3] < 0) break;
            }
        }
    } else {
        // the wave's 64 columns lie in one 128-column block: lane l looks at the flag of plane p0 + l, a ballot gives the live planes
        // (flag_shift: log2 of the columns a flag stands for - 7, or 6 when the owner sweep ran with one column per lane)
        const unsigned char* __restrict__ fl = colflag + (i >> flag_shift) * nseg;
        for (int p0 = 0; p0 < nseg; p0 += 64) {
            unsigned long long live = __ballot(p0 + lane < nseg && fl[p0 + lane] != 0);
            while (live) {
                const int s0 = p0 + __builtin_ctzll(live);
                live &= live - 1;
                const int s1 = live ? p0 + __builtin_ctzll(live) : -1;
                live &= live - 1;  // (0 stays 0)
                const float* __restrict__ o0 = fpart + (int64_t)s0 * 6 * ncap + i;
                const float* __restrict__ o1 = fpart + (int64_t)(s1 < 0 ? s0 : s1) * 6 * ncap + i;
                float v0[6], v1[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    v0[k] = o0[k * ncap];
                    v1[k] = o1[k * ncap];
                }
                merge(v0[0], v0[1], v0[2], v0[3], v0[4], v0[5]);
                if (s1 >= 0) merge(v1[0], v1[1], v1[2], v1[3], v1[4], v1[5]);
            }
        }
    }
    const double den = A * exp2(-(double)goff);  // underflows to 0 exactly where fp64 exp() does
    double c = 0.0;
    if (w > 0.0) c = pow(2.0 * M_PI * sigma2, dim * 0.5) * (w / (1.0 - w) * m_over_n);
    float b, p;
    double pd = 0.0, qn = 0.0;
    if (den == 0.0) {  // cpd.py:81: den = eps32, the column of P is all zero
        b = -INFINITY;
        p = 0.f;
    } else {
        const double tot = den + c;
        b = (float)(-log2(tot));
        pd = den / tot;
        p = (float)pd;
        qn = pd / A;
    }
    float cmin = 0.f;
    double a[kMomComp];
#pragma unroll
    for (int k = 0; k < kMomComp; ++k) a[k] = 0.0;
    if (valid) {
        reinterpret_cast<float*>(tgt4 + i)[3] = b;
        pt1[i] = p;
        colmin[i] = gmin;
        cmin = gmin;
        const float4 xf = tgt4[i];
        const double x[3] = {xf.x, xf.y, xf.z};
        double pz[3], xu = 0.0, xx = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pz[k] = pd * x[k] - qn * U[k];
            xu += x[k] * U[k];
            xx += x[k] * x[k];
        }
        a[0] = pd;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[1 + r] = pd * x[r];
            a[4 + r] = pz[r];
#pragma unroll
            for (int k = 0; k < 3; ++k) a[7 + 3 * r + k] = x[r] * pz[k];
        }
        a[16] = pd * xx + qn * (R - 2.0 * xu);
        a[22] = pd * xx;
    } else {
        b = 0.f;
    }
    block_reduce_store(a, mompart);
    {  // per group of 32 columns the largest of the minima, and the shard's largest (exactly as k_colfinal)
        const float gm = half_max(cmin);
        if ((threadIdx.x & 31) == 0) colmin_g[(int64_t)blockIdx.x * (kBlock / 32) + (threadIdx.x >> 5)] = gm;
        __shared__ float wg_max[kBlock / 32];
        if ((threadIdx.x & 31) == 0) wg_max[threadIdx.x >> 5] = gm;
        __syncthreads();
        if (threadIdx.x == 0) {
            float mx = wg_max[0];
#pragma unroll
            for (int k = 1; k < kBlock / 32; ++k) mx = fmaxf(mx, wg_max[k]);
            if (mx > 0.f) atomicMax(stat + 4 + slot, __float_as_uint(mx));
        }
    }
    if (gmeta) block_group_meta(0.f, 0.f, 0.f, b, b, false, gmeta);
}

// block partials of k_colfinal_fused -> MOMENTS in the layout k_mstep reads.  The sweep saw the TRANSFORMED source
// z = s R y + t; the rigid M-step wants sums over y: y = R^T (z - t) / s, so
//   Sy = R^T (Sz - S0 t) / s,   Sxy = (Sxz - Sx t^T) R / s,   tr Syy = (tr Szz - 2 t.Sz + S0 |t|^2) / s^2
// (R orthonormal: a rotation - checked on the host for the initial one, true by construction afterwards; the M-step only
// takes the trace of Syy for a rigid fit, cpd.py:179-182, so it goes to [16] and the other five entries stay 0).
__global__ __launch_bounds__(kRedBlock) void k_fused_final(const double* __restrict__ part, int nblk,
                                                           const double* __restrict__ params, double* __restrict__ moments) {
    __shared__ double sh[32][33];
    __shared__ double m[32];
    const int c = threadIdx.x & 31, slice = threadIdx.x >> 5;
    double sum = 0.0;
    if (c < kMomComp)
        for (int b = slice; b < nblk; b += 32) sum += part[(int64_t)b * kMomComp + c];
    sh[slice][c] = sum;
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 32; ++k) t += sh[k][threadIdx.x];
        m[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double S0 = m[0], s = params[12];
    const double t[3] = {params[9], params[10], params[11]};
    double tsz = 0.0, tt = 0.0;
    moments[0] = S0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        moments[1 + i] = m[1 + i];
        tsz += t[i] * m[4 + i];
        tt += t[i] * t[i];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double sy = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sy += params[3 * k + j] * (m[4 + k] - S0 * t[k]);  // (R^T)[j][k] = R[k][j]
        moments[4 + j] = sy / s;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) v += (m[7 + 3 * i + k] - m[1 + i] * t[k]) * params[3 * k + j];
            moments[7 + 3 * i + j] = v / s;
        }
    moments[16] = (m[16] - 2.0 * tsz + S0 * tt) / (s * s);
#pragma unroll
    for (int k = 17; k < 22; ++k) moments[k] = 0.0;
    moments[22] = m[22];
    moments[23] = 0.0;
}

__global__ __launch_bounds__(kBlock) void k_row_moments(const float* __restrict__ rowpart, int nseg, int64_t mcap,
                                                        int64_t m, const float4* __restrict__ src4,
                                                        const float4* __restrict__ z4, double* __restrict__ rowacc,
                                                        double* __restrict__ mompart,
                                                        const unsigned char* __restrict__ rowflag,
                                                        const float4* __restrict__ rorig, const QueueView qv, int lean) {
    if (qv.chunk) queue_reset(qv);
    // lean: the row pass left no residual sums e (k_rowpass_mfma<LEAN>: planes p1, ux, uy, uz only) - component 22,
    // sum_n pt1_n |x_n|^2, is filled in from the column side afterwards (k_xpx_columns)
    const bool has_e = !lean;
    double a[kMomComp];
#pragma unroll
    for (int c = 0; c < kMomComp; ++c) a[c] = 0.0;
    // grid-stride over the rows: few workgroups -> few partials for the single-block final reduction.  The trip count is the
    // same for the 64 lanes of a wave (`valid` masks the rows past the end): the queue consumer below talks across lanes.
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i - lane < m; i += (int64_t)gridDim.x * kBlock) {
        const bool valid = i < m;
        double p1 = 0, u[3] = {0, 0, 0}, e = 0;
        if (qv.chunk) {
            // The slots of the row's block of 128, [unit][5][128]: the wave's 64 rows share the block, so lane c fetches chunk
            // c's table entry once and the (first slot, units) pairs are handed round with readlane; the units are then
            // taken FOUR at a time (20 loads in flight), in order: chunk by chunk, unit by unit.
            const int2* __restrict__ cb = qv.chunk + (i >> 7) * qv.nchunk;
            for (int c0 = 0; c0 < qv.nchunk; c0 += 64) {
                const int2 mine = c0 + lane < qv.nchunk ? cb[c0 + lane] : make_int2(0, 0);
                const int lim = qv.nchunk - c0 < 64 ? qv.nchunk - c0 : 64;
                int c = -1, left = 0, next = 0;
                auto next_slot = [&]() -> int {  // (wave-uniform)
                    while (left == 0) {
                        if (++c >= lim) return -1;
                        next = __builtin_amdgcn_readlane(mine.x, c);
                        left = __builtin_amdgcn_readlane(mine.y, c);
                    }
                    --left;
                    return next++;
                };
                for (;;) {
                    int sl[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) sl[q] = next_slot();
                    if (sl[0] < 0) break;
                    float v[4][5];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float* __restrict__ o = rowpart + (int64_t)(sl[q] < 0 ? sl[0] : sl[q]) * 640 + (i & 127);
#pragma unroll
                        for (int k = 0; k < 5; ++k) v[q][k] = o[128 * k];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (sl[q] < 0) continue;
                        p1 += (double)v[q][0];
                        u[0] += (double)v[q][1];
                        u[1] += (double)v[q][2];
                        u[2] += (double)v[q][3];
                        e += (double)v[q][4];
                    }
                    if (sl[3] < 0) break;
                }
            }
        }
        // (128-row wave block, segment) partials the culled row pass never touched are absent (neither written nor
        // read): the wave fetches its block's 64 flag bytes once and walks the set bits (<= 64 planes)
        uint64_t live = qv.chunk ? 0ull : (nseg >= 64 ? ~0ull : ((1ull << nseg) - 1ull));
        if (rowflag && !qv.chunk) {
            const int wb = __builtin_amdgcn_readfirstlane((int)(i >> 7));
            const uint4* __restrict__ f = reinterpret_cast<const uint4*>(rowflag + (int64_t)wb * 64);
            uint64_t bits = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 v = f[q];
                const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int bb = 0; bb < 4; ++bb)
                        bits |= (uint64_t)((w4[k] >> (8 * bb)) & 1u) << (q * 16 + k * 4 + bb);
            }
            live &= bits;
        }
        while (live) {
            // two live segments per trip: ten independent loads in flight
            const int s = __builtin_ctzll(live);
            live &= live - 1;
            const int s2 = live ? __builtin_ctzll(live) : s;
            const double k2 = live ? 1.0 : 0.0;
            live &= live - 1;
            const float* __restrict__ o = rowpart + (int64_t)s * 5 * mcap + i;
            const float* __restrict__ o2 = rowpart + (int64_t)s2 * 5 * mcap + i;
            const float v0 = o[0], v1 = o[mcap], v2 = o[2 * mcap], v3 = o[3 * mcap], v4 = has_e ? o[4 * mcap] : 0.f;
            const float w0 = o2[0], w1 = o2[mcap], w2 = o2[2 * mcap], w3 = o2[3 * mcap], w4 = has_e ? o2[4 * mcap] : 0.f;
            p1 += (double)v0 + k2 * (double)w0;
            u[0] += (double)v1 + k2 * (double)w1;
            u[1] += (double)v2 + k2 * (double)w2;
            u[2] += (double)v3 + k2 * (double)w3;
            e += (double)v4 + k2 * (double)w4;
        }
        // reference point of the residual sums: the row's own z_m (VALU sweeps) or the origin of its 512-row block
        // (matrix-core sweeps) - the identities below hold for any reference
        const float4 zf = rorig ? rorig[i / prg::kMfmaWgPoints] : z4[i], yf = src4[i];
        const double z[3] = {zf.x, zf.y, zf.z};
        const double y[3] = {yf.x, yf.y, yf.z};
        double px[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = u[k] + p1 * z[k];  // exact identity: sum P x = sum P (x - z) + p1 z
        double t[kMomComp];
#pragma unroll
        for (int c = 0; c < kMomComp; ++c) t[c] = 0.0;
        row_moment_terms(t, p1, px, y);
        // sum_n pt1_n |x_n|^2 restricted to this row: sum_n P |x|^2 = p1 |z|^2 + 2 z.u + e
        t[22] = has_e ? p1 * (z[0] * z[0] + z[1] * z[1] + z[2] * z[2]) + 2.0 * (z[0] * u[0] + z[1] * u[1] + z[2] * u[2]) + e : 0.0;
        if (valid) {
#pragma unroll
            for (int c = 0; c < kMomComp; ++c) a[c] += t[c];
            rowacc[i] = p1;
            rowacc[mcap + i] = px[0];
            rowacc[2 * mcap + i] = px[1];
            rowacc[3 * mcap + i] = px[2];
        }
    }
    block_reduce_store(a, mompart);
}

// Lean matrix-core row pass: moments[22] = sum_n pt1_n |x_n|^2 from k_colfinal's per-workgroup partials (fixed order), scaled
// by (sum of the ROW sums p1) / (sum of the column sums pt1): the two differ by ~1e-6 (fp32 accumulation drops the far tail
// of a long sum), and the M-step's sigma2 subtracts quantities built from the row sums from this one.
__global__ __launch_bounds__(kBlock) void k_xpx_columns(const double* __restrict__ xpart, int nblk, double* __restrict__ moments) {
    __shared__ double sh[kBlock / 64][2];
    double x = 0.0, p = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kBlock) {
        x += xpart[2 * (int64_t)b];
        p += xpart[2 * (int64_t)b + 1];
    }
    const double wx = wave_sum(x), wp = wave_sum(p);
    if ((threadIdx.x & 63) == 0) {
        sh[threadIdx.x >> 6][0] = wx;
        sh[threadIdx.x >> 6][1] = wp;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tx = 0.0, tp = 0.0;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) {
            tx += sh[k][0];
            tp += sh[k][1];
        }
        moments[22] = tp > 0.0 ? tx * (moments[0] / tp) : tx;
    }
}

static QueueView queue_view(const SweepQueue& q, bool active) {
    QueueView v;
    v.chunk = active ? q.chunk.p : nullptr;
    v.nchunk = q.nchunk;
    v.ctrl = q.ctrl.p;
    v.pop_start = prg::kQueueWorkgroups * (prg::kSweepBlock / 64);
    v.cap_soft = q.cap_soft;
    return v;
}

// ---------------------------------------------------------------------------------------------
// layout of an E-step: segments, partial planes, engines that may run, buffer sizes (host arithmetic only)
// ---------------------------------------------------------------------------------------------
// Segment count for the streamed axis.  The grid should hold ~12.5k workgroups (~50k waves: enough to hide the
// scalar-load latency of the streams and, in the culled regime, short enough per-wave chains) whatever the size
// of the lane-owned cloud: C1 on one GPU -> 64 x 196 workgroups (best both dense and culled, tools/cull_floor.py);
// an 8-way target shard (12.5k local columns, 25 workgroups wide) -> ~200 short column-pass segments instead of 8
// long ones, which is what keeps a shard's E-step near 1/8 of the single-GPU time (tools/shard_profile2.py).
// Large clouds keep segments of >= 2048 streamed points (one ballot of group tests), at most 64 of them.
int auto_segments(int64_t nblk_x, int64_t stream_len, int quantum, int cap) {
    int64_t target = std::max<int64_t>(prg::ceil_div(12544, std::max<int64_t>(nblk_x, 1)),
                                       std::min<int64_t>(stream_len / 2048, 64));
    target = std::min<int64_t>(std::max<int64_t>(target, 1), cap);
    const int64_t seg = prg::round_up(prg::ceil_div(stream_len, target), quantum);
    return (int)prg::ceil_div(stream_len, seg);
}

// Culled sweeps: a workgroup = 128 lane points x 4 consecutive segments (one per wave, merged in LDS), so
// S segments cost S/4 partial planes.  Segments of 512 streamed points keep a wave's chain of dependent
// scalar loads short - the bound of a sparse E-step (tools/wave_trace.py) - and 256 segments (64 planes,
// the width of the row pass' touched-flag rows) are the cap; small problems get 256-point segments.
// [r3] Few owned blocks (a target shard's column pass, the row pass against a short shard) leave the chip with
// too few waves to hide a chain of 16 groups behind: below 65536 waves the segments are 256 points (8 groups) -
// 8 ranks at C1: E-step 0.245 -> 0.213 ms (mid), 0.124 -> 0.105 ms (late), tools/shard_segments.py.
int cull_segments(int64_t lane_points, int64_t stream_len, int64_t cap) {
    int64_t s = std::min<int64_t>(prg::ceil_div(stream_len, 512), cap);
    if (s * prg::ceil_div(lane_points, 128) < 65536) s = std::min<int64_t>(prg::ceil_div(stream_len, 256), cap);
    return (int)std::max<int64_t>(s, 1);
}

// Segments of a matrix-core launch once its chunk / tile masks skip work ([r5]).  The default grid fills the
// chip's 768 workgroup slots about once when there are few owned blocks (a target shard's column pass: 25 blocks x 30 segments
// of 14 chunks at 1/8 of C1) - fine while every chunk is needed, but a culled sweep then lasts as long as its busiest
// workgroup, which still needs its whole segment: rank 0 of 8 stayed at 0.31 ms from EM iteration 6 to 10 while one GPU went
// 1.78 -> 0.87 ms (profiles/r4_shard_window.log).  With >= 3 rounds of shorter segments the slots even the load out.
// 0: the default grid is already that deep (C1 on one GPU: 4.85 rounds), or PRG_MFMA_SEG pins the count.
// Since then a culling column launch also deals its chunks interleaved (EngineDecision::deal, k_colpass_mfma): the depth of the grid
// no longer decides how evenly a block's neighbourhood is spread over its workgroups, only how many workgroups share it.  One GPU at
// C1 keeps its 19 segments.  (Pinned to 32 / 48 / 64 / 96 with the interleaved deal, iterations 6 - 12 of the window took 6.90 / 6.93 /
// 7.09 / 7.28 ms against 7.06 - 7.15 at 19, profiles/mfma_deal_ab.log: a finer grid for one GPU's culling launches may be worth
// 0.2 ms, measured before the cloud's last block culled - DESIGN.md 8.)  The rule for shards stands as measured in round 5; it has
// not been re-measured with the new deal.
int mfma_fine_segments(int64_t owned, int64_t streamed, int max_planes) {
    const CpdEnv& env = prg::cpd_env();
    if (env.mfma_seg || env.fine_grid_off) return env.mfma_seg;
    const int64_t blocks = prg::ceil_div(owned, prg::kMfmaWgPoints), chunks = prg::ceil_div(streamed, 256);
    int64_t want = prg::ceil_div(3 * 768 + 256, blocks);
    want = std::min<int64_t>(std::min<int64_t>(want, chunks / 4), max_planes);
    return want > prg::mfma_planes(owned, streamed, 0) ? (int)want : 0;
}

// float2 elements of `planes` residual-form partial planes of the column pass: 6 floats per (plane, column) and, behind them
// (prg::resid_flags), one touched-flag byte per (block of `block_cols` columns, plane), with room for the flag kernels' over-read
int64_t resid_plane_elems(const prg_cpd& h, int planes, int block_cols) {
    return (int64_t)3 * planes * h.Ncap + (prg::ceil_div(h.N, block_cols) * planes + 64) / 8 + 8;
}

// Below how many evaluated pairs per owned point does a matrix-core sweep lose to the vector-pipe sweep?  The matrix-core sweeps
// stay while they evaluate enough pairs per owned point - counted by the sweeps themselves, one E-step back, so the switch
// follows the clouds' shape, their density and the size of this rank's shard instead of a fit in sigma2.  The count P (pairs)
// is compared with a two-line cost model of the engines (tools/mfma_vs_valu.py, profiles/r3_engine_switch_*.log):
//   matrix cores:  a workgroup owns 512 points and a segment of `cps` 256-point chunks of the other cloud, tau per
//                  chunk; in the dense regime some workgroup still needs its whole segment - cps x tau however
//                  much the others cull - and when the grid is deeper than the chip's 768 workgroup slots that
//                  workgroup may start late: + (1 - 768 / workgroups) x P x tau / (768 x 512 x 256)
//   vector pipe:   the evaluated 128 x 32 blocks are shared out evenly: c_v x P
// plus a difference `delta` of the fixed costs.  Leave when the vector pipe is shorter:
//   P < (cps x tau + delta) / (c_v - (1 - 768 / workgroups) x tau / (768 x 512 x 256))
// with  column pass  tau 12 us    c_v 0.200 ps  delta -15 us
//       row pass     tau 19.2 us  c_v 0.233 ps  delta  +8 us
// - per-kernel constants of this chip, the same for every cloud: surface, volume and 10:1:1 clouds of 12k ... 400k
// points and 1/2, 1/4, 1/8 shards of 100k all cross over within one EM iteration of what this predicts.  Host arithmetic only.
// (the model and its constants describe the DEFAULT grid, which is what the crossovers were measured on; the finer grid of a
// culling sweep only makes the matrix cores faster near the crossover - leaving at this bound is then slightly early, never late)
double engine_leave_below(int64_t owned, int64_t streamed, double tau, double delta, double c_v) {
    const int seg = prg::cpd_env().mfma_seg;
    // (segments as round 4 cut them: the rule the constants were fitted with, see mfma_chunks_per_seg_model)
    const int cps_i = seg ? prg::mfma_chunks_per_seg(owned, streamed, seg) : prg::mfma_chunks_per_seg_model(owned, streamed);
    const double cps = (double)cps_i;
    const double wgs = (double)prg::ceil_div(owned, prg::kMfmaWgPoints) * (double)prg::ceil_div(prg::ceil_div(streamed, 256), cps_i);
    const double late = std::max(0.0, 1.0 - 768.0 / wgs) * tau / (768.0 * 512.0 * 256.0);
    return std::max(0.0, cps * tau + delta) / (c_v - late) / (double)owned;  // pairs per owned point
}

// Lower end of the dense regime while a single sweep may run, as a multiple of the column pass' own bound.
// One fused sweep against the vector pipe's two: it stays ahead further down than the matrix-core column pass alone does
// (measured at C1, profiles/r4_fused_lower_bound.log: with the dense regime's lower end at 1.0 / 0.7 / 0.5 / 0.35 / 0.25 of the
// column pass' bound the window runs at 792 / 815 / 840 / 831 / 830 it/s (+-2 %): half of that bound is where the
// gain levels off; with it, and the fused factor of 256, C1 runs fused through EM iteration 14)
// [r5] what the fused sweep competes with below the dense regime is ONE vector-pipe sweep too (the residual-form column pass,
// DESIGN.md 3.1f), whose per-pair cost is above the plain column pass' the bound was fitted on - as the fused sweep's is
// above the matrix-core column pass': same command, lower end at 0.5 / 0.75 / 1.0 / 1.4 of the column pass' bound:
// 828 / 841 / 855 / 859 it/s (profiles/r5_fused_lower_bound.log); 1.4 hands over at EM iteration 12 of C1 (0.64 -> 0.57 ms)
// [r6] with the clouds in kd-tree order and the owner sweep below it the C1 window is flat from 1.0 to 2.8 (906 / 909 / 912 / 910
// it/s at 1.0 / 1.4 / 2.0 / 2.8, profiles/r6_fused_lower_bound.log: the optimum is bracketed); target shards, whose ranks leave
// the matrix cores at their own iteration, do better the later they leave: 8 ranks 4.10 -> 3.99 ms per window at 1.4 -> 1.0
// (0.7: 4.02), 4 ranks 6.51 -> 6.42.  1.0 it is.
// With culling launches dealt interleaved (and the cloud's last block culling too) the matrix cores are ahead of the owner sweep for
// two more iterations of C1 (13: 0.29 against 0.37 ms, 14: 0.24 against 0.28 ms at 0.5), but the first owner sweep behind them costs
// 0.015 - 0.025 ms more and the window does not resolve the rest: 949 / 946 / 949 / 941 it/s at 1.0 / 0.7 / 0.5 / 0.35, each +-1.5 %
// (profiles/mfma_deal_ab.log).  1.0 stays.
double fused_lower_bound_scale(bool allow_resid) {
    const double env = prg::cpd_env().fused_rcol_scale;
    return env > 0.0 ? env : allow_resid ? 1.0 : 0.5;
}

// Lean matrix-core row pass while mean |x|^2 / (sigma2 D) <= this.
// (tools/lean_error.py, profiles/r4_lean_error_rigid_100k_*.log: with the row-sum scaling of k_xpx_columns sigma2 stays
// within 2.7e-6 of the oracle's up to an amplification of 190 - 1.5e-6 at 56, 2.0e-6 at 85; tests/test_lean_gpu.py holds
// the forced pass to 1e-5 up to 128 with w = 0 / 0.1 and on a 2-rank shard.  64 makes every matrix-core row pass of C1 lean.)
constexpr double kLeanFactor = 64.0;

// the first sweep over the work queue after the matrix cores has no previous build to size its units from: about
// `bound` pairs per owned point are needed then - 32 groups per unit unless that overfills the queue (>= 250k points)
int first_queue_unit(double bound, int64_t owned, int64_t streamed) {
    const double groups = std::min(bound, (double)streamed) * (double)owned / (128.0 * prg::kGroup);
    int q = 32;
    while (groups / q > 0.75 * prg::kQueueMaxUnits && q < 256) q *= 2;
    return q;
}

double m_over_n(const prg_cpd* h) { return h->uniform_ratio > 0.0 ? h->uniform_ratio : (double)h->M / (double)h->Nglobal; }

}  // namespace

namespace prg {
double engine_col_bound(int64_t m, int64_t n_local) { return engine_leave_below(n_local, m, 12.0e-6, -15.0e-6, 0.200e-12); }
// Row pass, round 4: what competes near the crossover is the LEAN matrix-core row pass (no residual sums: 14.5 us per chunk
// instead of 19.2) against vector-pipe sweeps that skip at 2^-48 - re-measured from identical states on the surface at
// 30k / 50k / 100k / 250k points and on rank 0 of 2 / 4 / 8 at 100k (profiles/r4_engine_switch_*.log): the two cross at
// 18.6k / 13.4k / 18k / 37.5k and 12.4k / 6.3k / 5.3k evaluated targets per source point; tau 14.5 us, c_v 0.25 ps, delta -20 us
// put the bound within x1.24 of every one of them (round 3's constants left 2-2.5x too early after those two changes).  Where the
// row pass cannot run lean (amplification above the lean factor, prg_cpd_set_lean_factor(0), no prg_cpd_init_sums) round 3's
// constants apply: the decision kernel, which knows, picks between the two bounds (EngineArgs::r_row_bound / r_row_bound_full).
double engine_row_bound(int64_t m, int64_t n_local, bool lean) {
    return lean ? engine_leave_below(m, n_local, 14.5e-6, -20.0e-6, 0.250e-12) : engine_leave_below(m, n_local, 19.2e-6, 8.0e-6, 0.233e-12);
}

int ensure_mompart(prg_cpd* h) {
    const int64_t need = mompart_elems(*h);
    PRG_HIP(h->mompart.ensure(need, need));
    return PRG_OK;
}

void reduce_partials(prg_cpd* h, const double* part, int nblk, int ncomp, double* out, int off) {
    k_reduce_partials<<<1, kRedBlock, 0, h->stream>>>(part, nblk, ncomp, out, off);
}

int estep_layout(const prg_cpd& h, EstepLayout* out) {
    const CpdEnv& env = cpd_env();
    EstepLayout L;
    L.ra = h.r_col ? h.r_col : 2;
    L.rb = h.r_row ? h.r_row : 2;
    L.RA = L.ra < 0 ? -L.ra : L.ra;
    L.RB = L.rb < 0 ? -L.rb : L.rb;
    // Culled sweeps need both clouds Morton-sorted (compact waves / groups); they walk the stream in groups of 32.
    L.use_cull = h.opt_cull && h.perm_src.p && h.perm_tgt.p && h.r_col == 0 && h.r_row == 0;  // (segment counts stay tunable)
    // segment lengths are multiples of the loop trip (8 points, or 256 points = 8 groups); the pads absorb the
    // overshoot and the prefetch over-read of the last segment
    const int quantum = L.use_cull ? kSuper : 8;
    if (L.use_cull) {
        L.SA = h.seg_col ? h.seg_col : cull_segments(h.N, h.M, 1024);
        L.SB = h.seg_row ? h.seg_row : cull_segments(h.M, h.N, 256);  // (64 planes: the width of the touched-flag rows)
    } else {
        L.SA = h.seg_col ? h.seg_col : auto_segments(ceil_div(h.N, kBlock * L.RA), h.M, quantum, 256);
        L.SB = h.seg_row ? h.seg_row : auto_segments(ceil_div(h.M, kBlock * L.RB), h.N, quantum, 64);
    }
    // equal segments of a whole number of quanta: seg = round_up(len / S), S = ceil(len / seg)
    auto seg_of = [quantum](int64_t len, int s) { return (int)round_up(ceil_div(len, s), quantum); };
    L.segA = seg_of(h.M, L.SA);
    L.segB = seg_of(h.N, L.SB);
    L.SA = (int)ceil_div(h.M, L.segA);
    L.SB = (int)ceil_div(h.N, L.segB);
    while (L.SA > 1 && (int64_t)L.SA * L.segA + kOverRead > h.Mcap) --L.SA, L.segA = seg_of(h.M, L.SA);
    while (L.SB > 1 && (int64_t)L.SB * L.segB + kOverRead > h.Ncap) --L.SB, L.segB = seg_of(h.N, L.SB);
    PRG_REQUIRE((int64_t)L.SA * L.segA + kOverRead <= h.Mcap && (int64_t)L.SB * L.segB + kOverRead <= h.Ncap,
                PRG_ERR_STATE, "prg_cpd_estep: internal segmenting failure");
    // partial planes in HBM: one per segment, or one per four segments for the culled sweeps
    L.PA = L.use_cull ? (int)ceil_div(L.SA, 4) : L.SA;
    L.PB = L.use_cull ? (int)ceil_div(L.SB, 4) : L.SB;
    PRG_REQUIRE(!L.use_cull || L.PB <= 64, PRG_ERR_INVALID, "prg_cpd_estep: at most 256 row-pass segments with culling");

    // matrix-core sweeps (dense regime, decided per E-step): segments of whole 512-point chunks, one plane each
    // ... for clouds large enough that the sweeps are worth it: below ~8k points an E-step is launch bound whatever the
    // engine, and a 512-point patch of a small cloud spans most of it (the patch-local origin buys no precision)
    L.mfma_possible = L.use_cull && h.dense_engine > 0 && !h.srcw.p && (h.dense_engine >= 2 || (h.M >= 8192 && h.N >= 8192));
    // ... cut to fill the chip once (PRG_MFMA_SEG = 0) and, once the previous sweep skipped a tenth of its pairs, in >= 3 rounds
    // of shorter segments (mfma_fine_segments)
    L.seg_col_fine = L.mfma_possible ? mfma_fine_segments(h.N, h.M, 256) : 0;
    L.seg_row_fine = L.mfma_possible ? mfma_fine_segments(h.M, h.N, 64) : 0;
    // (planes of a launch cut as a grid of segments - default or fine - and of either way to cut it: grid or stream mode)
    const int col_grid_planes = L.mfma_possible ? std::max(mfma_planes(h.N, h.M, env.mfma_seg), mfma_planes(h.N, h.M, L.seg_col_fine)) : 0;
    const int row_grid_planes = L.mfma_possible ? std::max(mfma_planes(h.M, h.N, env.mfma_seg), mfma_planes(h.M, h.N, L.seg_row_fine)) : 0;
    L.PAm = L.mfma_possible ? std::max(col_grid_planes, mfma_stream_planes(h.N, h.M)) : 0;
    L.PBm = L.mfma_possible ? std::max(row_grid_planes, mfma_stream_planes(h.M, h.N)) : 0;
    // sparse regime: sweeps over a device-built work queue (cpd_sweeps_queue.hip) - partial results per unit, not per plane
    // ... when both clouds are large: the queue costs a build pass and leaves more partial results than the grid of culled
    // waves, which only pays off while a sweep is long (measured at C1: ahead with the target on 1 or 2 ranks, behind on 4 and 8)
    L.use_queue = L.use_cull && (h.sparse_engine == 2 || ((h.sparse_engine == 1 || h.sparse_engine == 3) && h.M >= 32768 && h.N >= 32768));
    // the single sweeps need: a caller that wants nothing but a rigid M-step's moments, unweighted sources, a rotation to map
    // the column-side sums back through
    const bool single_ok = h.moments_only && !h.nonrigid && !h.bcpd && h.init_rot_orthonormal;
    L.allow_fused = L.mfma_possible && single_ok;
    // the residual-form single sweep on the vector pipe: the same callers as the fused sweep, any sigma2, no
    // matrix cores needed
    L.allow_resid = L.use_cull && h.resid_sweep && single_ok && !h.srcw.p;
    // ... which the column block's owner runs ([r6] cpd_sweeps_owner.hip: the stream dealt out over PO parts x 8 waves per 128-column
    // block, cells found through the chunk / group hierarchy; prg_cpd_set_sparse_engine(0 / 2 / 3): round 5's grid / queue instead)
    L.use_owner = L.allow_resid && h.sparse_engine == 1 && !env.owner_off;
    L.PO = L.use_owner ? owner_planes(h.N, h.M) : 0;

    // Partial results of the column pass, in float2 elements, per engine that can run:
    const int64_t col_grid = (int64_t)L.PA * h.Ncap;                                      // (min, sum) per (plane, column)
    const int64_t col_mfma = (int64_t)L.PAm * h.Ncap;                                     // ... of a matrix-core launch
    const int64_t col_queue = L.use_queue ? queue_max_units(h.N, h.M) * 128 : 0;          // ... per (unit, column of its block of 128)
    const int64_t col_fused = L.allow_fused ? (int64_t)3 * col_grid_planes * h.Ncap : 0;  // 6 floats per (plane, column); never stream mode
    // (the residual form is sized for the ONE engine that runs it: with the work queue the vector pipe's column pass never goes
    // through the grid of planes)
    const int64_t col_resid = !L.allow_resid ? 0 : L.use_owner ? resid_plane_elems(h, L.PO, 64)
                              : L.use_queue ? 3 * col_queue : resid_plane_elems(h, L.PA, 128);
    L.colpart_elems = std::max({col_grid, col_mfma, col_queue, col_fused, col_resid});
    // ... of the row pass, in floats: 5 per (plane, row) + the touched flags (64 bytes per 128 rows), or 5 x 128 per unit
    const int64_t row_planes = (int64_t)std::max(L.PB, L.PBm) * 5 * h.Mcap + (h.Mcap >> 7) * 16;
    const int64_t row_queue = L.use_queue ? queue_max_units(h.M, h.N) * 640 : 0;
    L.rowpart_elems = std::max(row_planes, row_queue);
    // per-workgroup counters of evaluated (wave, group) blocks (prg_cpd_pair_counts): workgroups of the widest culled launch
    L.wgcount_elems = !L.use_cull ? 0 : std::max({ceil_div(h.N, 128) * L.PA, ceil_div(h.N, 64) * L.PO, ceil_div(h.M, 128) * L.PB,
                                                  ceil_div(h.N, kMfmaWgPoints) * L.PAm, ceil_div(h.M, kMfmaWgPoints) * L.PBm});
    L.mompart_elems = mompart_elems(h);
    *out = L;
    return PRG_OK;
}
}  // namespace prg

namespace {
// ---------------------------------------------------------------------------------------------
// the driver's steps
// ---------------------------------------------------------------------------------------------
int ensure_estep_buffers(prg_cpd* h, const EstepLayout& L) {
    PRG_HIP(h->colpart.ensure(L.colpart_elems, L.colpart_elems));
    PRG_HIP(h->rowpart.ensure(L.rowpart_elems, L.rowpart_elems));
    PRG_HIP(h->mompart.ensure(L.mompart_elems, L.mompart_elems));
    if (L.use_queue) PRG_TRY(prg::prepare_queues(h));
    if (L.wgcount_elems > h->wg_cap()) {  // ([0, wg_cap) column pass, [wg_cap, 2 wg_cap) row pass)
        if (h->wgcount.p) PRG_HIP(hipStreamSynchronize(h->stream));
        PRG_HIP(h->wgcount.reset(2 * L.wgcount_elems));
    }
    return PRG_OK;
}

// one fused kernel: transform, source motion, group boxes of the transformed cloud.  Non-rigid: z = y + G W with the
// parameter block's identity linear part (the fp64 sum is rounded once, transformation.py:101-102)
int transform_source(prg_cpd* h, int slot) {
    const double* disp = h->bcpd ? h->W.p : nullptr;
    if (h->nonrigid) PRG_TRY(prg::nonrigid_displacement(h, &disp));
    k_transform_linear<<<(unsigned)prg::ceil_div(h->M, kBlock), kBlock, 0, h->stream>>>(
        h->src4.p, h->z4.p, h->M, h->params, h->motion.p, slot, h->zmeta.p, h->srcw.p, disp, h->zchunk.p);  // pad-only blocks are static
    return PRG_OK;
}

// What the engine decision of one E-step came to (all false: vector pipe, two sweeps unless the residual form is allowed).
struct EstepEngines {
    bool use_mfma = false, row_mfma = false;  // column pass / row pass on the matrix cores
    bool first = false;                       // ... column pass without seeds (first E-step of a registration)
    bool fine = false;                        // ... with the per-wave group tests (some groups can be skipped by now)
    bool row_lean = false;                    // ... row pass without its residual sums (k_rowpass_mfma<LEAN>)
    bool fused = false;                       // ... ONE sweep for the whole E-step (rigid M-step moments from the column side)
    bool col_launched = false;                // the column pass (or the fused sweep) is already in the stream
};

// host -> decision kernel.  Also leaves the unit size of a first sweep over the work queue in the plan (it needs the bounds).
void fill_engine_args(prg_cpd* h, const EstepLayout& L, int slot, EngineArgs* out) {
    const CpdEnv& env = prg::cpd_env();
    EngineArgs ea;
    // size of the problem: the (replicated) source's bounding box or the local target's, whichever is larger - a
    // target shard is a small patch, and every rank should leave the dense regime at the same sigma2
    ea.ext2 = std::max(h->sext2, h->text2);
    ea.r_col_bound = env.r_col > 0.0 ? env.r_col : h->dense_bound > 0.0 ? h->dense_bound : prg::engine_col_bound(h->M, h->N);
    ea.r_col_bound_fused = ea.r_col_bound * fused_lower_bound_scale(L.allow_resid);
    ea.r_row_bound = env.r_row > 0.0 ? env.r_row : prg::engine_row_bound(h->M, h->N, true);
    ea.r_row_bound_full = env.r_row > 0.0 ? env.r_row : prg::engine_row_bound(h->M, h->N, false);  // (the device knows which applies)
    ea.streamed_col = (double)h->M;
    ea.streamed_row = (double)h->N;
    h->q_first_col = first_queue_unit(ea.r_col_bound, h->N, h->M);
    h->q_first_row = first_queue_unit(ea.r_row_bound, h->M, h->N);
    ea.owned_col = (double)h->N;
    ea.owned_row = (double)h->M;
    ea.work = h->eng_work;
    ea.tsum = h->tsum_local;  // (prg_cpd_init_sums: sums of the LOCAL target; zeros if it was never called: not lean)
    ea.dim = h->D;
    ea.lean_factor = h->lean_factor >= 0.0 ? h->lean_factor : env.lean_factor >= 0.0 ? env.lean_factor : kLeanFactor;
    ea.deal_mode = env.mfma_deal;
    ea.deal_below = env.mfma_deal_below;
    ea.fused_allowed = L.allow_fused ? 1 : 0;
    ea.resid_allowed = L.allow_resid ? 1 : 0;
    ea.fused_factor = env.fused_factor >= 0.0 ? env.fused_factor : h->fused_factor;
    ea.reset = h->eng.reset ? 1 : 0;
    for (int k = 0; k < 6; ++k) ea.tbox[k] = h->tbox[k];
    ea.slot = slot;
    ea.have_colmin = h->have_colmin ? 1 : 0;
    ea.forced = h->dense_engine >= 2 ? 1 : 0;
    ea.seq = (unsigned)h->estep_count;  // (already incremented: never 0, the mailbox's initial value)
    ea.dev = &h->eng_dev.p->decision;
    ea.host = h->eng_host_dev;
    *out = ea;
}

// Dense regime on the matrix cores?  Decided per E-step from numbers only the device has at this point - sigma2, the
// source motion of this transform, the largest column minimum of the previous E-step - so the device
// decides (last thread of k_chunk_meta_bbox) and the host neither reads back nor synchronises: it launches the column
// pass of the engine the PREVIOUS E-step used right behind the decision kernel (guarded: the launch returns at once if
// the decision names the other engine), then polls the mapped mailbox while that launch runs and enqueues the rest of
// the E-step behind it - the queue never drains.  Once sigma2 has fallen to where the culled vector sweeps skip most
// of the pairs the registration stays on them and nothing is asked any more.
int decide_engines(prg_cpd* h, const EstepLayout& L, int slot, bool cull_seed, hipEvent_t* ev, EstepEngines* out) {
    EstepEngines d;
    *out = d;
    if (!L.mfma_possible || h->eng.mfma_off) {
        if (ev) PRG_HIP(hipEventRecord(ev[1], h->stream));
        return PRG_OK;
    }
    PRG_TRY(prg::ensure_engine_state(h));
    EngineArgs ea;
    fill_engine_args(h, L, slot, &ea);
    h->eng.reset = false;
    // chunk boxes of this E-step's transformed source (the matrix-core sweeps cull with them), its bounding box, and
    // the decision
    prg::launch_chunk_meta_bbox(h, &ea);
    if (ev) PRG_HIP(hipEventRecord(ev[1], h->stream));
    // segments of a matrix-core column pass: finer once the previous decision saw the sweep skip a tenth of its pairs
    auto seg_col = [&]() { return h->eng.grid_fine && L.seg_col_fine ? L.seg_col_fine : prg::cpd_env().mfma_seg; };
    const bool pred = h->eng.pred_col != 0, pred_fused = L.allow_fused && h->eng.pred_fused != 0;
    const bool vector_grid = !L.use_queue && !L.use_owner;  // the vector pipe's column pass would be the grid of culled waves
    if (pred_fused)  // (the single sweep of a rigid iteration, if the previous E-step ran it)
        prg::launch_fused_mfma(h, seg_col(), !h->have_colmin, false, h->eng.deal != 0, ea.dev);
    else if (pred)  // (stream mode if the previous decision found nothing to skip: the dense regime)
        prg::launch_colpass_mfma(h, seg_col(), !h->have_colmin, false, h->eng.deal != 0, ea.dev, h->mfma_stream && h->eng.pred_fine == 0 && !h->eng.grid_fine);
    else if (vector_grid)
        prg::launch_colpass_cull(h, L.SA, L.segA, cull_seed, ea.dev, L.allow_resid);
    // (pred == vector pipe with the work queue / the owner sweep: nothing goes out ahead - inside the dense regime that engine only
    // runs when the bracket of the column minima is too wide for the matrix-core offsets, a handful of E-steps at most)
    PRG_HIP(hipGetLastError());
    // the answer: a few microseconds after the transform has finished, long before the column pass has
    volatile EngineDecision* mb = h->eng_host.p;
    hipError_t werr;
    const bool got = prg::wait_mailbox(&mb->seq, ea.seq, h->stream, &werr);
    PRG_HIP(werr);
    PRG_REQUIRE(got, PRG_ERR_HIP, "prg_cpd_estep: the engine decision never reached the host");
    d.use_mfma = mb->col != 0;
    d.first = mb->first != 0;
    d.row_mfma = mb->row != 0;
    d.fine = mb->fine != 0;
    d.row_lean = d.row_mfma && mb->lean != 0;
    d.fused = L.allow_fused && mb->fused != 0;
    if (!mb->dense) h->eng.mfma_off = true;
    // the previous matrix-core column pass skipped a tenth of its pairs: its masks are at work, cut the grid finer from here on
    // (the same count, on the device, switches the chunk deal of this E-step's launch: EngineDecision::deal)
    h->eng.grid_fine = !d.first && (double)mb->r_col < 0.9 * (double)h->M;
    if (prg::cpd_env().debug_engine)
        fprintf(stderr, "[engine] sigma2 %.4e nk*ext2 %.1f pairs per owned point col %.0f (bound %.0f) row %.0f (bound %.0f) motion %.3e cmax %.3e nk*width %.1f "
                        "nk*far2 %.1f have_colmin %d -> col %d (first %d, launched ahead: %s) row %d fine %d\n",
                (double)mb->sigma2, (double)mb->nk_ext2, (double)mb->r_col, ea.r_col_bound, (double)mb->r_row, ea.r_row_bound,
                (double)mb->motion, (double)mb->cmax,
                (double)mb->nk_width, (double)mb->nk_far2, (int)h->have_colmin, (int)d.use_mfma, (int)d.first,
                pred == d.use_mfma ? "yes" : "NO", (int)d.row_mfma, (int)d.fine);
    // which of the three guarded launches (fused sweep / matrix-core column pass / culled column pass) went out ahead, and
    // was it the one the decision names?
    if (pred_fused)
        d.col_launched = d.fused;
    else if (pred)
        d.col_launched = d.use_mfma && !d.fused;
    else
        d.col_launched = !d.use_mfma && vector_grid;
    h->eng.pred_col = d.use_mfma ? 1 : 0;
    h->eng.pred_fine = d.fine ? 1 : 0;
    h->eng.pred_fused = d.fused ? 1 : 0;
    h->eng.deal = mb->deal;
    if (!d.col_launched && d.fused) {  // (the guarded launch has returned at once; rare: the engine changes a few times per registration)
        prg::launch_fused_mfma(h, seg_col(), d.first, d.fine, h->eng.deal != 0, ea.dev);
        d.col_launched = true;
    } else if (!d.col_launched && d.use_mfma) {
        prg::launch_colpass_mfma(h, seg_col(), d.first, d.fine, h->eng.deal != 0, ea.dev, h->mfma_stream && !d.fine && !h->eng.grid_fine);
        d.col_launched = true;
    }
    *out = d;
    return PRG_OK;
}

// Which vector-pipe engine ran the column pass, if the decision step had not launched it already.
struct ColumnPass {
    bool owner = false, queue = false;
};
int column_pass(prg_cpd* h, const EstepLayout& L, const EstepEngines& d, bool resid, bool cull_seed, ColumnPass* out) {
    ColumnPass cp;
    cp.owner = !d.col_launched && resid && L.use_owner;
    cp.queue = !d.col_launched && L.use_queue && !cp.owner;
    if (d.col_launched) {
    } else if (cp.owner)
        prg::launch_colpass_owner(h, cull_seed, L.PO);
    else if (cp.queue)
        PRG_TRY(prg::launch_colpass_queue(h, cull_seed, h->qcol_live ? 0 : h->q_first_col, resid));
    else if (L.use_cull)
        prg::launch_colpass_cull(h, L.SA, L.segA, cull_seed, nullptr, resid);
    else if (L.ra < 0)
        prg::launch_colpass_scalar(h, L.RA, L.SA, L.segA);
    else
        prg::launch_colpass_packed(h, L.RA, L.SA, L.segA);
    *out = cp;
    return PRG_OK;
}

// End of every E-step: the one exchange step of the path when the target is sharded over ranks - partial
// moments -> moments, on this stream - and what the plan remembers of the E-step.
int finish_estep(prg_cpd* h, double w, bool col_queue, bool row_queue, bool rowacc_valid) {
    PRG_HIP(hipGetLastError());
    if (h->comm) {
        // (the E-step's 24 sums only: [24..27] hold the target sums prg_cpd_init_sums has already made global)
        PRG_TRY(prg::comm_all_reduce_f64(h->comm, h->moments, kMomComp, h->stream));
        if (h->nonrigid && rowacc_valid) PRG_TRY(prg::comm_all_reduce_f64(h->comm, h->rowacc.p, 4 * h->Mcap, h->stream));
    }
    h->qcol_live = col_queue;
    h->qrow_live = row_queue;
    h->have_estep = true;
    h->estep_state_live = true;
    h->rowacc_valid = rowacc_valid;
    h->have_colmin = true;  // colmin now describes the z4 of this E-step (motion is measured against it)
    h->last_w = w;
    return PRG_OK;
}

// A single-sweep E-step (fused on the matrix cores, or the residual form on the vector pipe): den_n / pt1_n / the next E-step's
// seeds AND the moments come out of one merge kernel; no row pass, no per-point block
int single_sweep_tail(prg_cpd* h, const EstepLayout& L, const EstepEngines& d, const ColumnPass& cp, bool resid, double w, int slot,
                      hipEvent_t* ev) {
    const int nblk = (int)prg::ceil_div(h->N, kBlock);
    float* const colmin_g = h->colmin.p + h->Ncap;
    const float* part = reinterpret_cast<const float*>(h->colpart.p);
    if (!resid) {  // fused: per-column (A, B, E) relative to the block origins
        k_colfinal_fused<<<nblk, kBlock, 0, h->stream>>>(h->tgt4.p, part, h->mfma_col_planes, h->Ncap, h->N, h->pt1.p, h->params, w, m_over_n(h),
                                                         h->D, h->colmin.p, colmin_g, h->tmeta.p, d.first ? 2 : 1, h->motion.p, slot, h->corig.p,
                                                         h->mompart.p);
    } else if (cp.queue) {  // per-column (A, U, R), residuals against the column's own x_n: in the slots of the queue's units
        k_colfinal_resid<true><<<nblk, kBlock, 0, h->stream>>>(h->tgt4.p, part, 0, h->Ncap, h->N, h->pt1.p, h->params, w, m_over_n(h), h->D,
                                                               h->colmin.p, colmin_g, h->tmeta.p, h->motion.p, slot, nullptr,
                                                               queue_view(h->qcol, true), h->mompart.p, 7);
    } else {  // ... in planes with their touched flags; a flag stands for 128 columns, or for 64 when the owner sweep ran one per lane
        const int planes = cp.owner ? L.PO : L.PA;
        k_colfinal_resid<false><<<nblk, kBlock, 0, h->stream>>>(h->tgt4.p, part, planes, h->Ncap, h->N, h->pt1.p, h->params, w, m_over_n(h), h->D,
                                                                h->colmin.p, colmin_g, h->tmeta.p, h->motion.p, slot, prg::resid_flags(h, planes),
                                                                queue_view(h->qcol, false), h->mompart.p,
                                                                cp.owner && prg::owner_cols_per_lane() == 1 ? 6 : 7);
    }
    if (ev) {
        PRG_HIP(hipEventRecord(ev[3], h->stream));
        PRG_HIP(hipEventRecord(ev[4], h->stream));
    }
    k_fused_final<<<1, kRedBlock, 0, h->stream>>>(h->mompart.p, nblk, h->params, h->moments);
    if (ev) PRG_HIP(hipEventRecord(ev[5], h->stream));
    h->wg_row = 0;
    h->dense_pairs_row = 0.0;
    return finish_estep(h, w, cp.queue, false, false);
}

int two_sweep_tail(prg_cpd* h, const EstepLayout& L, const EstepEngines& d, const ColumnPass& cp, double w, int slot, hipEvent_t* ev) {
    const int mfma_seg = prg::cpd_env().mfma_seg;
    // (lean matrix-core row pass: no residual sums - sum pt1 |x|^2 goes from k_colfinal's partials to k_xpx_columns)
    double* xpart = h->mompart.p + (int64_t)prg::mom_blocks(*h) * kMomComp;
    k_colfinal<<<grid1(h->N), kBlock, 0, h->stream>>>(h->tgt4.p, h->colpart.p, d.use_mfma ? h->mfma_col_planes : L.PA, h->Ncap, h->N, h->pt1.p, h->params, w,
                                                      m_over_n(h), h->D, h->colmin.p, h->colmin.p + h->Ncap,
                                                      L.use_cull ? h->tmeta.p : nullptr, d.use_mfma ? (d.first ? 2 : 1) : 0, h->motion.p, slot,
                                                      queue_view(h->qcol, cp.queue), d.row_lean ? xpart : nullptr);
    if (ev) PRG_HIP(hipEventRecord(ev[3], h->stream));
    const bool row_queue = !d.row_mfma && L.use_queue;
    if (d.row_mfma)
        prg::launch_rowpass_mfma(h, h->eng.grid_fine && L.seg_row_fine ? L.seg_row_fine : mfma_seg, d.fine, d.row_lean, h->mfma_stream && !d.fine && !h->eng.grid_fine);
    else if (row_queue)
        PRG_TRY(prg::launch_rowpass_queue(h, h->qrow_live ? 0 : h->q_first_row));
    else if (L.use_cull)
        prg::launch_rowpass_cull(h, L.SB, L.segB);
    else if (L.rb < 0)
        prg::launch_rowpass_scalar(h, L.RB, L.SB, L.segB);
    else
        prg::launch_rowpass_packed(h, L.RB, L.SB, L.segB);
    if (ev) PRG_HIP(hipEventRecord(ev[4], h->stream));
    const int nblk = (int)std::min<int64_t>(prg::ceil_div(h->M, kBlock), 1024);
    const int row_planes = d.row_mfma ? h->mfma_row_planes : L.PB;
    k_row_moments<<<nblk, kBlock, 0, h->stream>>>(h->rowpart.p, row_planes, h->Mcap, h->M, h->src4.p, h->z4.p, h->rowacc.p,
                                                  h->mompart.p,
                                                  L.use_cull ? reinterpret_cast<const unsigned char*>(h->rowpart.p + (int64_t)row_planes * 5 * h->Mcap)
                                                             : nullptr,
                                                  d.row_mfma ? h->rorig.p : nullptr, queue_view(h->qrow, row_queue), d.row_lean ? 1 : 0);
    // (folding this single-block reduction into the last-finishing workgroup of k_row_moments was measured in round 3:
    // +25 us - that workgroup's 256 threads read the ~400 partial rows through L2 in a few dependent rounds, the 1024
    // threads of this launch do it in 5 us including the launch)
    k_reduce_partials<<<1, kRedBlock, 0, h->stream>>>(h->mompart.p, nblk, kMomComp, h->moments, 0);
    if (d.row_lean) k_xpx_columns<<<1, kBlock, 0, h->stream>>>(xpart, (int)prg::ceil_div(h->N, kBlock), h->moments);
    if (ev) PRG_HIP(hipEventRecord(ev[5], h->stream));
    return finish_estep(h, w, cp.queue, row_queue, true);
}

}  // namespace

// layout -> buffers -> transform -> engine decision -> column pass -> merge tail
int prg::estep_impl(prg_cpd* h, double w, hipEvent_t* ev) {
    PRG_REQUIRE(h && h->have_source && h->have_target, PRG_ERR_STATE, "prg_cpd_estep: clouds not set");
    PRG_REQUIRE(w >= 0.0 && w < 1.0, PRG_ERR_INVALID, "prg_cpd_estep: w must be in [0, 1) (got %g)", w);
    PRG_ENTER_AS("prg_cpd_estep", h->device);
    EstepLayout L;
    PRG_TRY(estep_layout(*h, &L));
    PRG_TRY(ensure_estep_buffers(h, L));

    if (ev) PRG_HIP(hipEventRecord(ev[0], h->stream));
    const int slot = (int)(h->estep_count & 1);
    ++h->estep_count;
    PRG_TRY(transform_source(h, slot));
    const bool cull_seed = h->have_colmin && !h->srcw.p;  // the seed bound assumes unweighted distances
    h->wg_col_pairs = h->wg_row_pairs = 128.0 * prg::kGroup;  // a (wave, group) block of the culled vector-pipe sweeps
    EstepEngines d;
    PRG_TRY(decide_engines(h, L, slot, cull_seed, ev, &d));
    // the vector pipe's column pass of an E-step that feeds nothing but a rigid M-step is the residual-form single sweep
    const bool resid = L.allow_resid && !d.use_mfma;
    const bool single = d.fused || resid;
    h->last_estep_mfma = d.use_mfma;
    h->last_estep_fused = single;
    // (a single-sweep E-step has no row pass: nothing to report for it)
    h->last_estep_row_mfma = d.row_mfma && !single;
    h->last_estep_row_lean = d.row_lean && !single;
    ColumnPass cp;
    PRG_TRY(column_pass(h, L, d, resid, cull_seed, &cp));
    if (ev) PRG_HIP(hipEventRecord(ev[2], h->stream));
    return single ? single_sweep_tail(h, L, d, cp, resid, w, slot, ev) : two_sweep_tail(h, L, d, cp, w, slot, ev);
}
