// FilterReg rigid EM iteration on MI355X (gfx950): the plan (clouds, state, E-step over the permutohedral lattice of
// lattice.hip) and the M-step kernels (point-to-point: weighted Kabsch reduction; point-to-plane: 6 x 6 twist solve).
//
// Reference behaviour (neka-nat/probreg v0.3.7):
//   E-step    probreg/filterreg.py:78-108        M-step  probreg/filterreg.py:158-196 (pt2pt)
//   Kabsch    probreg/cc/kabsch.cc:6-109
#include <math.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

#include <stdio.h>
#include <stdlib.h>

#include "morton.h"
#include "prg_device.h"
#include "prg_common.h"
#include "small_linalg.h"
#include "lattice.h"
#include "fr_plan.h"

using prg::DevBuf;
using prg::FrFeat;
using prg::Lattice;

// =============================================================================================
// FilterReg plan
// =============================================================================================
struct prg_filterreg {
    Lattice L;
    Lattice& ctx() { return L; }  // device and stream (plan_base.h)
    int64_t M = 0, N = 0;
    int D = 0;
    // (the device buffers own their memory, dev_buf.h: deleting the plan releases them)
    DevBuf<double> src;      // [M][4] fp64 source (x, y, z, 0)
    DevBuf<double> tgt;      // [N][4] fp64 target
    DevBuf<double> nrm;      // [N][3] fp64 target normals (point-to-plane objective), optional
    int ch = 5;              // value channels: 1 | y(3) | |y|^2  (+ normal(3) when normals are set)
    DevBuf<double> ts;       // [M][4] fp64 transformed source
    DevBuf<float> vin;       // [M+N][ch] values (source rows zero)
    DevBuf<float> vout;      // [M][ch] filtered m0, m1(3), m2 (, nx(3))
    DevBuf<double> state;    // [64]: 0..8 rot, 9..11 t, 12 sigma2, 13 q, 14 nonzero count, 15 sigma2_new
    DevBuf<double> part;     // block partials
    int64_t part_blocks = 0;
    bool slice_pending = false;  // the last E-step stopped before its slice step (lat_filter defer_slice); see fr_flush_slice
    std::vector<int> tgt_order;  // Morton order of the target (kernel position -> caller's index); see prg_fr_set_target
    DevBuf<int> ref_pos;         // [N] device: caller's index -> kernel position (the ordered splat walks the caller's order)
    DevBuf<int> src_perm;        // [M] device: kernel position -> caller's index of the (Morton-sorted) source; empty: caller's order
    bool have_src = false, have_tgt = false, have_estep = false;
    FrFeat prod;             // feature producer handed to the embedding kernels
    int last_blur = 1;       // with_blur of the previous E-step: which lattice the next one tries first
    int route[4] = {0, 0, 0, 0};  // how the last E-step chose its lattice (prg_fr_last_route); route[0] == 0: none yet
    // deformable kinematic model (filterreg_kinematic.hip, reached through fr_plan.h)
    std::vector<int> src_order;            // host copy of src_perm (empty: caller's order)
    const double* src_override = nullptr;  // non-null during prg_fr_kinematic_estep: the skinned source stands in for `src`
    void* kin = nullptr;                   // skinning context, owned by the plan ...
    void (*kin_free)(void*) = nullptr;     // ... and released through this
};

namespace {

constexpr int kBlock = 256;
constexpr int kFrComp = 32;  // 0 sw,1-3 sw*m,4-6 sw*t,7 sw2,8-10 sw2*m,11-13 sw2*t,14-22 sw2*m*t^T,23 q,24 s2num,25 m0m0,26 cnt

// values [M+N][ch]: source rows 0; target rows (1, y, |y|^2 [, normal])   (filterreg.py:92-105)
__global__ __launch_bounds__(kBlock) void k_fr_values(const double* __restrict__ tgt, const double* __restrict__ nrm,
                                                      int64_t m, int64_t n, int dim, int ch,
                                                      float* __restrict__ vin) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m + n) return;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i >= m) {
        const double* y = tgt + (i - m) * 4;  // (4 doubles per point)
        double s = 0.0;
        v[0] = 1.0f;
        for (int k = 0; k < dim; ++k) {
            v[1 + k] = (float)y[k];
            s += y[k] * y[k];
        }
        v[4] = (float)s;
        if (ch == 8)
            for (int k = 0; k < 3; ++k) v[5 + k] = (float)nrm[(i - m) * 3 + k];
    }
    for (int k = 0; k < ch; ++k) vin[i * ch + k] = v[k];
}

// per-point M-step terms (filterreg.py:163-182, 190-195) -> block partials [nblk][kFrComp]
// c = w/(1-w) * n/m * (2 sigma2 pi)^(dim/2)   (filterreg.py:164), evaluated on the device: no host round trip
__device__ __forceinline__ double fr_uniform_c(double wfac, int dim, double sigma2) {
    return wfac * pow(2.0 * sigma2 * M_PI, dim * 0.5);
}

__device__ void fr_finish_body(const double* __restrict__ part, int nblk, int dim, int update_sigma2, double min_sigma2,
                               double* __restrict__ state);

// SLICE: the lattice's slice step (permutohedral.cpp:521-528 / :586-592: barycentric interpolation of the D + 1 enclosing
// vertices, the reference's two arithmetic flavours per channel) is done HERE, per source point, instead of in a k_slice launch
// of its own: the five filtered values of a point go to `vout` (prg_fr_get_estep) and straight into the point's M-step terms -
// one launch, one dependent-launch gap and one 22 MB re-read less per EM iteration.  The Kabsch finish is a launch of its own
// again (k_fr_finish): folded into the last workgroup of this kernel (round 3) it doubled the kernel's registers (200 VGPRs:
// 2 waves per SIMD for the 512 workgroups that never run it) and cost 57 us where the two launches take 16 + 12.
// M1SEQ (2-D clouds): the reference filters m1 as y.shape[1] = 2 channels, and at most two channels go through seqCompute.
template <bool SLICE, bool M1SEQ = false>
__global__ __launch_bounds__(kBlock) void k_fr_terms(const float* __restrict__ vout_in, float* __restrict__ vout_w, int ch,
                                                     const int* __restrict__ offset, const float* __restrict__ bary,
                                                     const float* __restrict__ vals, float alpha,
                                                     const double* __restrict__ ts, int64_t m, int dim, double wfac,
                                                     const double* __restrict__ state, double* __restrict__ part) {
    __shared__ double sh[4][kFrComp];
    double a[kFrComp];
#pragma unroll
    for (int k = 0; k < kFrComp; ++k) a[k] = 0.0;
    const double sigma2 = state[12];
    const double c = fr_uniform_c(wfac, dim, sigma2);
    // grid-stride: a few hundred workgroups, each thread sums several points before the (32-component) reduction
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        float f[5];
        if (SLICE) {  // (ch == 5, fr_seq_mask: channels 0 and 4 follow seqCompute, 1..3 sseCompute unless M1SEQ - see k_slice)
            const int d1 = dim + 1;
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = 0.f;
            for (int r = 0; r < d1; ++r) {
                const int o = offset[i * d1 + r] + 1;
                const float w = bary[i * d1 + r];
                const float* __restrict__ v = vals + (int64_t)o * 5;
                const float wa = __fmul_rn(w, alpha);
                f[0] = __fadd_rn(f[0], __fmul_rn(__fmul_rn(w, v[0]), alpha));
                if (M1SEQ) {  // (channel 3 is zero in 2-D)
                    f[1] = __fadd_rn(f[1], __fmul_rn(__fmul_rn(w, v[1]), alpha));
                    f[2] = __fadd_rn(f[2], __fmul_rn(__fmul_rn(w, v[2]), alpha));
                } else {
                    f[1] = __fadd_rn(f[1], __fmul_rn(wa, v[1]));
                    f[2] = __fadd_rn(f[2], __fmul_rn(wa, v[2]));
                    f[3] = __fadd_rn(f[3], __fmul_rn(wa, v[3]));
                }
                f[4] = __fadd_rn(f[4], __fmul_rn(__fmul_rn(w, v[4]), alpha));
            }
#pragma unroll
            for (int k = 0; k < 5; ++k) vout_w[i * 5 + k] = f[k];
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = vout_in[i * ch + k];
        }
        const float m0 = f[0];
        if (m0 != 0.f) {
            const double2 za = reinterpret_cast<const double2*>(ts)[2 * i], zb = reinterpret_cast<const double2*>(ts)[2 * i + 1];
            const double z[3] = {za.x, za.y, zb.x};  // (4 doubles per point)
            const float m1[3] = {f[1], f[2], f[3]};
            const float m2 = f[4];
            float tg[3];  // m1m0 = m1 / m0 in float32 (:172)
            for (int k = 0; k < 3; ++k) tg[k] = k < dim ? __fdiv_rn(m1[k], m0) : 0.f;
            const double m0m0 = (double)m0 / ((double)m0 + c);       // :173
            const double dr = sqrt(m0m0 / sigma2);                    // :174
            const double w = (double)(float)dr;                        // the Kabsch binding casts to float32
            const double w2 = w * w;
            double mod[3];
            for (int k = 0; k < 3; ++k) mod[k] = k < dim ? (double)(float)z[k] : 0.0;
            a[0] += w;
            a[7] += w2;
            double r2 = 0.0, zz = 0.0, zm1 = 0.0;
            for (int k = 0; k < 3; ++k) {
                a[1 + k] += w * mod[k];
                a[4 + k] += w * (double)tg[k];
                a[8 + k] += w2 * mod[k];
                a[11 + k] += w2 * (double)tg[k];
                for (int j = 0; j < 3; ++j) a[14 + 3 * k + j] += w2 * mod[k] * (double)tg[j];
                if (k < dim) {
                    const double rx = dr * (z[k] - (double)tg[k]);
                    r2 += rx * rx;
                    zz += z[k] * z[k];
                    zm1 += z[k] * (double)m1[k];
                }
            }
            a[23] += sqrt(r2);                                                          // q term, :181-182
            a[24] += ((double)m0 * zz - 2.0 * zm1 + (double)m2) / ((double)m0 + c);    // :192-194
            a[25] += m0m0;
            a[26] += 1.0;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kFrComp; ++k) {
        const double s = wave_sum(a[k]);
        if (lane == 0) sh[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kFrComp)
        part[(int64_t)blockIdx.x * kFrComp + threadIdx.x] =
            sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

// point-to-plane M-step terms (filterreg.py:183-186 -> cc/point_to_plane.cc:6-32): per point with m0 != 0
//   v = t_source (float32), t = m1/m0, n = nx/m0, w = sqrt(m0m0/sigma2) (float32),
//   residual = n.(t - v), jac = [v x n, n]:  ata += w jac jac^T (21 upper entries), atb += w residual jac,
//   r_sum += w^2 residual^2.  comps: [0..20] ata, [21..26] atb, [27] r_sum, [28] sigma2 numerator, [29] m0m0, [30] count
__global__ __launch_bounds__(kBlock) void k_fr_terms_pt2pl(const float* __restrict__ vout, const double* __restrict__ ts,
                                                           int64_t m, double wfac, const double* __restrict__ state,
                                                           double* __restrict__ part) {
    __shared__ double sh[4][kFrComp];
    double a[kFrComp];
#pragma unroll
    for (int k = 0; k < kFrComp; ++k) a[k] = 0.0;
    const double sigma2 = state[12];
    const double c = fr_uniform_c(wfac, 3, sigma2);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += (int64_t)gridDim.x * kBlock) {
        const float m0 = vout[i * 8];
        if (m0 != 0.f) {
            const double z[3] = {ts[i * 4], ts[i * 4 + 1], ts[i * 4 + 2]};  // (4 doubles per point)
            double v[3], t[3], n[3];
            double zz = 0.0, zm1 = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float m1 = vout[i * 8 + 1 + k];
                v[k] = (double)(float)z[k];
                t[k] = (double)__fdiv_rn(m1, m0);
                n[k] = (double)__fdiv_rn(vout[i * 8 + 5 + k], m0);
                zz += z[k] * z[k];
                zm1 += z[k] * (double)m1;
            }
            const double m0m0 = (double)m0 / ((double)m0 + c);
            const double w = (double)(float)sqrt(m0m0 / sigma2);
            const double residual = n[0] * (t[0] - v[0]) + n[1] * (t[1] - v[1]) + n[2] * (t[2] - v[2]);
            const double jac[6] = {v[1] * n[2] - v[2] * n[1], v[2] * n[0] - v[0] * n[2], v[0] * n[1] - v[1] * n[0],
                                   n[0], n[1], n[2]};
            int idx = 0;
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int q = r; q < 6; ++q) a[idx++] += w * jac[r] * jac[q];
#pragma unroll
            for (int r = 0; r < 6; ++r) a[21 + r] += w * residual * jac[r];
            a[27] += w * w * residual * residual;
            a[28] += ((double)m0 * zz - 2.0 * zm1 + (double)vout[i * 8 + 4]) / ((double)m0 + c);
            a[29] += m0m0;
            a[30] += 1.0;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kFrComp; ++k) {
        const double s = wave_sum(a[k]);
        if (lane == 0) sh[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kFrComp)
        part[(int64_t)blockIdx.x * kFrComp + threadIdx.x] =
            sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

// sum over the block partials of component c for this thread's slice (8 slices of 32 components): four independent
// accumulators keep four loads in flight - a single dependent chain of ~250 loads costs ~60 us on its own
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nblk, int slice, int c) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int b = slice;
    for (; b + 24 < nblk; b += 32) {
        s0 += part[(int64_t)b * kFrComp + c];
        s1 += part[(int64_t)(b + 8) * kFrComp + c];
        s2 += part[(int64_t)(b + 16) * kFrComp + c];
        s3 += part[(int64_t)(b + 24) * kFrComp + c];
    }
    for (; b < nblk; b += 8) s0 += part[(int64_t)b * kFrComp + c];
    return (s0 + s1) + (s2 + s3);
}

// 6 x 6 SPD solve (the reference uses Eigen's LDLT on the upper triangle), twist -> Rodrigues rotation
// (se3_op.py:21-56), composition with the previous transform, optional sigma2 update.  One workgroup.
__global__ __launch_bounds__(kBlock) void k_fr_finish_pt2pl(const double* __restrict__ part, int nblk,
                                                            int update_sigma2, double min_sigma2,
                                                            double* __restrict__ state) {
    __shared__ double sh[8][32];
    __shared__ double mom[32];
    const int c = threadIdx.x & 31, slice = threadIdx.x >> 5;
    sh[slice][c] = sum_partials(part, nblk, slice, c);
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
        for (int k = 0; k < 8; ++k) t += sh[k][threadIdx.x];
        mom[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    state[14] = mom[30];
    if (mom[30] == 0.0) {
        state[13] = nan("");
        state[16] = 0.0;
        return;
    }
    state[16] = 1.0;
    // Cholesky solve of ata tw = atb (static indices)
    double A[6][6], bvec[6], tw[6];
    {
        int idx = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = r; q < 6; ++q) { A[r][q] = mom[idx]; A[q][r] = mom[idx]; ++idx; }
#pragma unroll
        for (int r = 0; r < 6; ++r) bvec[r] = mom[21 + r];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < 6; ++k) d -= (k < j) ? A[j][k] * A[j][k] : 0.0;
        d = sqrt(fmax(d, 1e-300));
        A[j][j] = d;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            if (i <= j) continue;
            double t = A[i][j];
#pragma unroll
            for (int k = 0; k < 6; ++k) t -= (k < j) ? A[i][k] * A[j][k] : 0.0;
            A[i][j] = t / d;
        }
    }
    double yv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double t = bvec[i];
#pragma unroll
        for (int k = 0; k < 6; ++k) t -= (k < i) ? A[i][k] * yv[k] : 0.0;
        yv[i] = t / A[i][i];
    }
#pragma unroll
    for (int ii = 0; ii < 6; ++ii) {
        const int i = 5 - ii;
        double t = yv[i];
#pragma unroll
        for (int k = 0; k < 6; ++k) t -= (k > i) ? A[k][i] * tw[k] : 0.0;
        tw[i] = t / A[i][i];
    }
    // twist -> (rotation, translation), se3_op.py:21-41
    double tr[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    const double twd = sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
    if (twd != 0.0) {
        const double n0 = tw[0] / twd, n1 = tw[1] / twd, n2 = tw[2] / twd;
        const double cc = cos(twd), ss = sin(twd), oc = 1.0 - cc;
        tr[0][0] = cc + oc * n0 * n0;      tr[0][1] = oc * n0 * n1 - ss * n2; tr[0][2] = oc * n0 * n2 + ss * n1;
        tr[1][0] = oc * n1 * n0 + ss * n2; tr[1][1] = cc + oc * n1 * n1;      tr[1][2] = oc * n1 * n2 - ss * n0;
        tr[2][0] = oc * n2 * n0 - ss * n1; tr[2][1] = oc * n2 * n1 + ss * n0; tr[2][2] = cc + oc * n2 * n2;
    }
    // rot = tr @ rot_p ; t = t_p @ tr^T + tw[3:]   (se3_op.py:44-56)
    double rp[3][3], tp[3], rn[3][3], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        tp[i] = state[9 + i];
#pragma unroll
        for (int j = 0; j < 3; ++j) rp[i][j] = state[3 * i + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double tt = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) r += tr[i][k] * rp[k][j];
            rn[i][j] = r;
            tt += tr[i][j] * tp[j];
        }
        tn[i] = tt + tw[3 + i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        state[9 + i] = tn[i];
#pragma unroll
        for (int j = 0; j < 3; ++j) state[3 * i + j] = rn[i][j];
    }
    state[13] = mom[27];  // q = r_sum
    state[18] = mom[27];  // ... of the last iteration that had anything to fit (a later all-zero one overwrites [13] with NaN)
    state[19] += 1.0;
    state[17] = state[12];
    state[15] = update_sigma2 ? mom[28] / (3.0 * mom[29]) : state[12];
    if (min_sigma2 >= 0.0) state[12] = fmax(state[15], min_sigma2);  // negative: do not advance (see k_fr_finish)
}

// weighted Kabsch from moments (cc/kabsch.cc:6-109): mom[0] sw, [1..3] sw*model, [4..6] sw*target, [7] sw2,
// [8..10] sw2*model, [11..13] sw2*target, [14..22] sw2*model*target^T.  Centroids use w, the covariance w^2.
__device__ void kabsch_from_moments(const double* mom, int dim, double (&dr)[3][3], double (&dt)[3]) {
    for (int i = 0; i < 3; ++i) {
        dt[i] = 0.0;
        for (int j = 0; j < 3; ++j) dr[i][j] = (i == j) ? 1.0 : 0.0;
    }
    const double sw = mom[0];
    if (sw != 0.0) {
        double mc[3], tc[3], H[3][3];
        for (int k = 0; k < 3; ++k) { mc[k] = mom[1 + k] / sw; tc[k] = mom[4 + k] / sw; }
        const double sw2 = mom[7];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j)
                H[i][j] = (mom[14 + 3 * i + j] - mc[i] * mom[11 + j] - mom[8 + i] * tc[j] + sw2 * mc[i] * tc[j]) / sw2;
        if (dim == 3) {
            double U[3][3], V[3][3], sv[3];
            prg::jacobi_svd(H, 3, U, V, sv);
            const double dd = prg::det3(U, 3) * prg::det3(V, 3);  // det(U V), kabsch.cc:48
            double c[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {  // the correction goes on the smallest singular value (static indices only)
                bool is_min = true;
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j != k && (sv[j] < sv[k] || (sv[j] == sv[k] && j < k))) is_min = false;
                c[k] = is_min ? dd : 1.0;
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    double r = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) r += c[k] * V[i][k] * U[j][k];  // V diag U^T
                    dr[i][j] = r;
                }
        } else {
            const double ang = atan2(H[0][1] - H[1][0], H[0][0] + H[1][1]);  // kabsch.cc:98
            dr[0][0] = dr[1][1] = cos(ang);
            dr[0][1] = -sin(ang);
            dr[1][0] = sin(ang);
        }
        for (int i = 0; i < 3; ++i) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += dr[i][k] * mc[k];
            dt[i] = tc[i] - r;
        }
    }
}

// weighted Kabsch from the moments (cc/kabsch.cc:6-109) + composition (filterreg.py:180) - one workgroup
__global__ __launch_bounds__(kBlock) void k_fr_finish(const double* __restrict__ part, int nblk, int dim,
                                                      int update_sigma2, double min_sigma2,
                                                      double* __restrict__ state) {
    fr_finish_body(part, nblk, dim, update_sigma2, min_sigma2, state);
}

__device__ void fr_finish_body(const double* __restrict__ part, int nblk, int dim, int update_sigma2, double min_sigma2,
                               double* __restrict__ state) {
    __shared__ double sh[8][32];
    __shared__ double mom[32];
    const int c = threadIdx.x & 31, slice = threadIdx.x >> 5;
    sh[slice][c] = sum_partials(part, nblk, slice, c);
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
        for (int k = 0; k < 8; ++k) t += sh[k][threadIdx.x];
        mom[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    state[14] = mom[26];
    if (mom[26] == 0.0) {  // every m0 == 0: keep the previous transform, q = None (:167-168)
        state[13] = nan("");
        state[16] = 0.0;
        return;
    }
    state[16] = 1.0;
    double dr[3][3], dt[3];
    kabsch_from_moments(mom, dim, dr, dt);
    // rot = dr @ rot_p ; t = t_p @ dr^T + dt   (filterreg.py:180)
    double rp[3][3], tp[3], rn[3][3], tn[3];
    for (int i = 0; i < 3; ++i) {
        tp[i] = state[9 + i];
        for (int j = 0; j < 3; ++j) rp[i][j] = state[3 * i + j];
    }
    for (int i = 0; i < 3; ++i) {
        double tt = 0.0;
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
            for (int k = 0; k < 3; ++k) r += dr[i][k] * rp[k][j];
            rn[i][j] = r;
            tt += dr[i][j] * tp[j];
        }
        tn[i] = tt + dt[i];
    }
    for (int i = 0; i < 3; ++i) {
        state[9 + i] = tn[i];
        for (int j = 0; j < 3; ++j) state[3 * i + j] = rn[i][j];
    }
    state[13] = mom[23];
    state[18] = mom[23];  // q of the last iteration that had anything to fit (a later all-zero one overwrites [13] with NaN)
    state[19] += 1.0;     // ... and how many of those there were since prg_fr_set_state
    state[17] = state[12];                                               // sigma2 this step was computed with
    state[15] = update_sigma2 ? mom[24] / (3.0 * mom[25]) : state[12];  // :192-195 (3.0 hard-coded there)
    // self._sigma2 = max(res.sigma2, min_sigma2), :140 - for every legal min_sigma2 (0 included); a NEGATIVE value
    // is the explicit "leave the device sigma2 alone" request of the stand-alone M-step entry points
    if (min_sigma2 >= 0.0) state[12] = fmax(state[15], min_sigma2);
}

// caller-supplied E-step arrays -> the [m][ch] value layout and the [m][3] fp64 transformed source the M-step
// kernels read (prg_fr_mstep_from_arrays)
__global__ __launch_bounds__(kBlock) void k_fr_pack_estep(const double* __restrict__ tsrc, const float* __restrict__ m0,
                                                          const float* __restrict__ m1, const float* __restrict__ m2,
                                                          const float* __restrict__ nx, int64_t m, int dim, int ch,
                                                          double* __restrict__ ts, float* __restrict__ vout) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    for (int k = 0; k < 4; ++k) ts[i * 4 + k] = k < dim ? tsrc[i * dim + k] : 0.0;  // (4 doubles per point)
    float* o = vout + i * ch;
    o[0] = m0[i];
    for (int k = 0; k < 3; ++k) o[1 + k] = k < dim ? m1[i * dim + k] : 0.f;
    o[4] = m2 ? m2[i] : 0.f;
    if (ch == 8)
        for (int k = 0; k < 3; ++k) o[5 + k] = nx[i * 3 + k];
}

// out[perm[i]][0 .. ncols) = vout[i][col0 .. col0 + ncols): the plan's per-source-point values back in the caller's order
__global__ __launch_bounds__(kBlock) void k_fr_columns(const float* __restrict__ vout, int ch, int col0, int ncols,
                                                       const int* __restrict__ perm, int64_t m, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int64_t j = perm ? perm[i] : i;
    for (int k = 0; k < ncols; ++k) out[j * ncols + k] = vout[i * ch + col0 + k];
}

// stand-alone Kabsch: moments of (model, target, weight) float32 clouds -> partials [nblk][kFrComp]
__global__ __launch_bounds__(kBlock) void k_kabsch_terms(const float* __restrict__ model,
                                                         const float* __restrict__ target,
                                                         const float* __restrict__ weight, int64_t n, int dim,
                                                         double* __restrict__ part) {
    __shared__ double sh[4][kFrComp];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double a[kFrComp];
#pragma unroll
    for (int k = 0; k < kFrComp; ++k) a[k] = 0.0;
    if (i < n) {
        const double w = weight[i], w2 = w * w;
        double mod[3] = {0, 0, 0}, tg[3] = {0, 0, 0};
        for (int k = 0; k < dim; ++k) { mod[k] = model[i * dim + k]; tg[k] = target[i * dim + k]; }
        a[0] = w;
        a[7] = w2;
        for (int k = 0; k < 3; ++k) {
            a[1 + k] = w * mod[k];
            a[4 + k] = w * tg[k];
            a[8 + k] = w2 * mod[k];
            a[11 + k] = w2 * tg[k];
            for (int j = 0; j < 3; ++j) a[14 + 3 * k + j] = w2 * mod[k] * tg[j];
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kFrComp; ++k) {
        const double s = wave_sum(a[k]);
        if (lane == 0) sh[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kFrComp)
        part[(int64_t)blockIdx.x * kFrComp + threadIdx.x] =
            sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

__global__ __launch_bounds__(kBlock) void k_kabsch_finish(const double* __restrict__ part, int nblk, int dim,
                                                          double* __restrict__ out) {
    __shared__ double sh[8][32];
    __shared__ double mom[32];
    const int c = threadIdx.x & 31, slice = threadIdx.x >> 5;
    sh[slice][c] = sum_partials(part, nblk, slice, c);
    __syncthreads();
    if (threadIdx.x < 32) {
        double t = 0.0;
        for (int k = 0; k < 8; ++k) t += sh[k][threadIdx.x];
        mom[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double dr[3][3], dt[3];
    kabsch_from_moments(mom, dim, dr, dt);
    for (int i = 0; i < 3; ++i) {
        out[9 + i] = dt[i];
        for (int j = 0; j < 3; ++j) out[3 * i + j] = dr[i][j];
    }
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------
// FilterReg plan
// ---------------------------------------------------------------------------------------------
int prg_fr_create(prg_filterreg** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream, [](prg_filterreg* h) -> int {
        PRG_HIP(h->state.reset(64));
        (void)hipMemsetAsync(h->state.p, 0, 64 * sizeof(double), h->L.stream);
        h->L.fx_scale_static = true;  // the plan's value array (target moments) only changes in fr_alloc
        return PRG_OK;
    });
}

int prg_fr_destroy(prg_filterreg* h) {
    return prg::destroy_handle(h, [](prg_filterreg* p) {  // (the lattice's and the plan's buffers release themselves)
        if (p->kin) p->kin_free(p->kin);
    });
}

// the buffers that depend on both clouds
static int fr_alloc_both(prg_filterreg* h) {
    if (!(h->have_src && h->have_tgt)) return PRG_OK;
    const int64_t tot = h->M + h->N;
    h->ts.release(); h->vin.release(); h->vout.release(); h->part.release();  // (all four go before the first comes back)
    h->L.fx_scale_key = nullptr;  // new values: the fixed-point scales are recomputed by the next filter call
    PRG_HIP(h->ts.reset(h->M * 4));  // (x, y, z, 0) per point
    PRG_HIP(h->vin.reset(tot * 8));
    PRG_HIP(h->vout.reset(h->M * 8));
    h->part_blocks = std::min<int64_t>(prg::ceil_div(h->M, kBlock), 512);  // grid-stride M-step term kernels
    PRG_HIP(h->part.reset(h->part_blocks * kFrComp));
    k_fr_values<<<(unsigned)prg::ceil_div(tot, kBlock), kBlock, 0, h->L.stream>>>(h->tgt.p, h->nrm.p, h->M, h->N, h->D,
                                                                                  h->ch, h->vin.p);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

// `have`: the caller's flag for the cloud it has just stored - not set if this fails, so no E-step runs over missing buffers
static int fr_alloc(prg_filterreg* h, bool* have) {
    *have = true;
    h->have_estep = false;
    const int st = fr_alloc_both(h);
    if (st != PRG_OK) *have = false;
    return st;
}

int prg_fr_set_source(prg_filterreg* h, const double* source_hd, int64_t m, int dim) {
    PRG_REQUIRE(h && source_hd, PRG_ERR_INVALID, "prg_fr_set_source: NULL argument");
    PRG_REQUIRE(m > 0 && (dim == 2 || dim == 3), PRG_ERR_INVALID, "prg_fr_set_source: need m > 0, dim in {2,3}");
    PRG_REQUIRE(!h->have_tgt || h->D == dim, PRG_ERR_INVALID, "prg_fr_set_source: dim mismatch with target");
    PRG_ENTER(h->L.device);
    PRG_HIP(hipStreamSynchronize(h->L.stream));
    if (h->kin) {  // skinning weights belong to the previous source
        h->kin_free(h->kin);
        h->kin = nullptr;
    }
    h->have_src = false;  // until the new cloud is on the device
    PRG_HIP(h->src.reset(m * 4));  // (x, y, z, 0) per point: 16-byte accesses in k_embed
    h->src_perm.release();
    static const bool sort_source = getenv("PRG_FR_SOURCE_ORDER") == nullptr;  // (set: keep the caller's order, as in round 2)
    {
        // The source is stored in Morton order like the target: with the lattice's vertices created by a sample spread over
        // both clouds (every 16th point, lat_build), the other points only LOOK vertices up, and neighbouring lanes of a
        // sorted cloud look up the same few table lines.  Every per-point output crosses the ABI through src_perm.
        std::vector<double> host((size_t)m * dim), padded((size_t)m * 4, 0.0);
        PRG_HIP(hipMemcpy(host.data(), source_hd, host.size() * sizeof(double), hipMemcpyDefault));
        std::vector<int> order;
        if (sort_source && m >= 4096) order = prg::morton_order(host.data(), m, dim);
        for (int64_t i = 0; i < m; ++i) {
            const int64_t j = order.empty() ? i : order[(size_t)i];
            for (int k = 0; k < dim; ++k) padded[(size_t)i * 4 + k] = host[(size_t)j * dim + k];
        }
        if (!order.empty()) {
            PRG_HIP(h->src_perm.reset(m));
            PRG_HIP(hipMemcpyAsync(h->src_perm.p, order.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->L.stream));
        }
        PRG_HIP(hipMemcpyAsync(h->src.p, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, h->L.stream));
        PRG_HIP(hipStreamSynchronize(h->L.stream));
        h->src_order = order;
    }
    h->M = m;
    h->D = dim;
    return fr_alloc(h, &h->have_src);
}

int prg_fr_set_target(prg_filterreg* h, const double* target_hd, int64_t n, int dim) {
    PRG_REQUIRE(h && target_hd, PRG_ERR_INVALID, "prg_fr_set_target: NULL argument");
    PRG_REQUIRE(n > 0 && (dim == 2 || dim == 3), PRG_ERR_INVALID, "prg_fr_set_target: need n > 0, dim in {2,3}");
    PRG_REQUIRE(!h->have_src || h->D == dim, PRG_ERR_INVALID, "prg_fr_set_target: dim mismatch with source");
    PRG_ENTER(h->L.device);
    PRG_HIP(hipStreamSynchronize(h->L.stream));
    h->have_tgt = false;  // until the new cloud is on the device
    PRG_HIP(h->tgt.reset(n * 4));  // (x, y, z, 0) per point
    // The target is stored in Morton order: the splat works on 2048 consecutive target points per workgroup, and
    // spatially close points share lattice vertices, so the workgroup-private LDS table absorbs most updates and
    // the flush touches few global vertices.  Every E-step output is per SOURCE point, so no order leaks out.
    std::vector<double> host((size_t)n * dim), sorted((size_t)n * 4, 0.0);
    PRG_HIP(hipMemcpy(host.data(), target_hd, host.size() * sizeof(double), hipMemcpyDefault));
    h->tgt_order = prg::morton_order(host.data(), n, dim);
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < dim; ++k) sorted[(size_t)i * 4 + k] = host[(size_t)h->tgt_order[i] * dim + k];
    PRG_HIP(hipMemcpyAsync(h->tgt.p, sorted.data(), sorted.size() * sizeof(double), hipMemcpyHostToDevice, h->L.stream));
    // ... and the splat still adds every vertex' terms up in the CALLER's point order (the reference's): caller index -> kernel position
    std::vector<int> inv((size_t)n);
    for (int64_t i = 0; i < n; ++i) inv[(size_t)h->tgt_order[i]] = (int)i;
    PRG_HIP(h->ref_pos.reset(n));
    PRG_HIP(hipMemcpyAsync(h->ref_pos.p, inv.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->L.stream));
    PRG_HIP(hipStreamSynchronize(h->L.stream));
    h->N = n;
    h->D = dim;
    h->nrm.release();  // normals belong to the previous target
    h->ch = 5;
    return fr_alloc(h, &h->have_tgt);
}

int prg_fr_set_state(prg_filterreg* h, const double* rot9, const double* t3, double sigma2) {
    PRG_REQUIRE(h && rot9 && t3, PRG_ERR_INVALID, "prg_fr_set_state: NULL argument");
    PRG_REQUIRE(sigma2 > 0.0, PRG_ERR_INVALID, "prg_fr_set_state: sigma2 must be > 0 (got %g)", sigma2);
    PRG_ENTER(h->L.device);
    double buf[20];
    for (int i = 0; i < 9; ++i) buf[i] = rot9[i];
    for (int i = 0; i < 3; ++i) buf[9 + i] = t3[i];
    buf[12] = sigma2;
    for (int i = 13; i < 20; ++i) buf[i] = 0.0;
    buf[15] = sigma2;
    PRG_HIP(hipMemcpyAsync(h->state.p, buf, sizeof(buf), hipMemcpyHostToDevice, h->L.stream));
    PRG_HIP(hipStreamSynchronize(h->L.stream));
    h->last_blur = 1;  // a (re)started registration begins with a large sigma2: try the blurred lattice first
    return PRG_OK;
}

// Which channels of the fused filter pass follow the reference's seqCompute (bit k set) and which its sseCompute: the
// reference filters m0 and m2 alone (one channel: seqCompute) and m1 as one filter of y.shape[1] channels - three take
// sseCompute, the two of a 2-D cloud seqCompute (permutohedral.cpp picks seqCompute up to two channels).  Normals: sseCompute.
static unsigned fr_seq_mask(const prg_filterreg* h) { return h->D == 2 ? 0x1Fu : 0x11u; }

int prg_fr_estep(prg_filterreg* h, double alpha, int* lattice_size, int* with_blur) {
    PRG_REQUIRE(h && h->have_src && h->have_tgt, PRG_ERR_STATE, "prg_fr_estep: clouds not set");
    PRG_ENTER(h->L.device);
    const int64_t tot = h->M + h->N;
    // features are produced inside the embedding kernels (transform, division by sigma, float32 cast)
    h->have_estep = false;  // (a failure below leaves no half-built lattice behind for an M-step)
    h->route[0] = 0;
    h->prod = FrFeat{h->src_override ? h->src_override : h->src.p, h->tgt.p, h->state.p, h->ts.p, h->M, h->D};
    h->L.prod = &h->prod;
    h->L.ref_pos = h->ref_pos.p;
    int blur = 1;
    // filterreg.py:90-91: the blurred lattice is used only if it has at most N * alpha vertices.  The answer is exact
    // every time; what changes with the previous E-step's answer is which lattice is built FIRST:
    //   previous blurred     -> the blurred lattice, whole (one synchronisation); if it came out too large, the other one;
    //   previous not blurred -> the non-blurred lattice, whole, while a 1/16 subset hashed with the blur scaling proves
    //                           that the blurred one is still too large (same synchronisation); if the proof fails, the
    //                           staged decision of round 1 (rare: sigma2 would have to grow again).
    const double thr = (double)h->N * alpha;
    const int64_t decide = thr >= 0.0 && thr < 2.0e9 ? (int64_t)floor(thr) : -1;
    bool done = false;
    int route = 0, builds = 0;  // (prg_fr_last_route)
    if (h->last_blur == 0 && decide >= 0 && tot >= 4096) {
        PRG_TRY(prg::lat_side_stage(&h->L, tot, h->D));
        PRG_TRY(prg::lat_build(&h->L, tot, h->D, 0));
        ++builds;
        if (h->L.side_overflow == 0 && h->L.side_size > decide) {
            blur = 0;
            done = true;
            route = 3;
        }
    }
    if (!done) {
        const int64_t decide_above = h->last_blur == 1 ? -1 : decide;
        PRG_TRY(prg::lat_build(&h->L, tot, h->D, 1, decide_above));
        ++builds;
        const bool rejected = !h->L.built || (double)h->L.size > thr;
        // Route 4 needs the first sixteenth alone to exceed the threshold.  With tot >= 4096 that sixteenth is the side
        // stage's sample under the same scaling, which has just failed to exceed it - so only an overflow of the side table
        // (a probe chain of more than 4096 slots in a table a quarter full at the most) leads here.
        if (decide_above >= 0) route = !h->L.built ? 4 : (rejected ? 6 : 5);
        else route = rejected ? 2 : 1;
        if (rejected) {
            blur = 0;
            PRG_TRY(prg::lat_build(&h->L, tot, h->D, 0));
            ++builds;
        }
    }
    h->last_blur = blur;
    // one fused 5-channel pass: channels 0 (m0) and 4 (m2) are single-channel filters in the reference
    // (seqCompute arithmetic), channels 1..3 (m1) its 3-channel filter (sseCompute arithmetic) - fr_seq_mask
    // (point-to-point plans, ch == 5: the slice step waits for its consumer - the M-step slices inside its terms kernel)
    h->slice_pending = h->ch == 5;
    PRG_TRY(prg::lat_filter(&h->L, h->vin.p, h->ch, h->M, h->M, fr_seq_mask(h), h->vout.p, h->slice_pending));  // normals (ch 5..7): 3-channel filter
    if (lattice_size) *lattice_size = h->L.size;
    if (with_blur) *with_blur = blur;
    h->have_estep = true;
    h->route[1] = builds;
    h->route[2] = h->L.attempts;
    h->route[3] = route >= 3 && tot >= 4096 ? 1 : 0;  // the decision looked at a sixteenth of the points first
    h->route[0] = route;
    return PRG_OK;
}

int prg_fr_last_route(prg_filterreg* h, int* out4) {
    PRG_REQUIRE(h && out4, PRG_ERR_INVALID, "prg_fr_last_route: NULL argument");
    PRG_REQUIRE(h->route[0] != 0, PRG_ERR_STATE, "prg_fr_last_route: no E-step has been run");
    for (int i = 0; i < 4; ++i) out4[i] = h->route[i];
    return PRG_OK;
}

static int fr_flush_slice(prg_filterreg* h);
}  // extern "C"

// what filterreg_kinematic.hip sees of a plan (fr_plan.h)
namespace prg {
int fr_view(prg_filterreg* h, FrView* v, bool flush_slice) {
    if (flush_slice && h->have_estep) PRG_TRY(fr_flush_slice(h));
    v->device = h->L.device;
    v->stream = h->L.stream;
    v->M = h->M; v->N = h->N; v->D = h->D; v->ch = h->ch;
    v->src = h->src.p; v->ts = h->ts.p; v->vout = h->vout.p; v->state = h->state.p;
    v->src_order = h->src_order.empty() ? nullptr : h->src_order.data();
    v->have_src = h->have_src; v->have_tgt = h->have_tgt; v->have_estep = h->have_estep;
    v->kin = &h->kin;
    v->kin_free = &h->kin_free;
    return PRG_OK;
}
int fr_estep_moved(prg_filterreg* h, const double* moved, double alpha, int* lattice_size, int* with_blur) {
    h->src_override = moved;
    const int st = prg_fr_estep(h, alpha, lattice_size, with_blur);
    h->src_override = nullptr;
    return st;
}
}  // namespace prg

extern "C" {
// the E-step's deferred slice, for every consumer of `vout` other than the point-to-point M-step
static int fr_flush_slice(prg_filterreg* h) {
    if (!h->slice_pending) return PRG_OK;
    h->slice_pending = false;
    return prg::lat_slice(&h->L, h->L.pend_vals, h->L.pend_alpha, h->ch, h->M, fr_seq_mask(h), h->vout.p);
}

// columns [col0, col0 + ncols) of the filtered values, one row per source point in the CALLER's order -> out_hd
static int fr_fetch_columns(prg_filterreg* h, int col0, int ncols, float* out_hd) {
    hipStream_t st = h->L.stream;
    PRG_TRY(fr_flush_slice(h));
    PRG_HIP(h->L.io.ensure(h->M * ncols, h->M * ncols));
    k_fr_columns<<<(unsigned)prg::ceil_div(h->M, kBlock), kBlock, 0, st>>>(h->vout.p, h->ch, col0, ncols, h->src_perm.p, h->M, h->L.io.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(out_hd, h->L.io.p, (size_t)h->M * ncols * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

int prg_fr_get_estep(prg_filterreg* h, float* m0_hd, float* m1_hd, float* m2_hd) {
    PRG_REQUIRE(h && h->have_estep, PRG_ERR_STATE, "prg_fr_get_estep: no E-step has been run");
    PRG_ENTER(h->L.device);
    if (m0_hd) PRG_TRY(fr_fetch_columns(h, 0, 1, m0_hd));
    if (m1_hd) PRG_TRY(fr_fetch_columns(h, 1, h->D, m1_hd));
    if (m2_hd) PRG_TRY(fr_fetch_columns(h, 4, 1, m2_hd));
    return PRG_OK;
}

static int fr_read_state(prg_filterreg* h, double* out_host, int count) {
    hipStream_t st = h->L.stream;
    PRG_HIP(h->L.pinned.ensure(64, hipHostMallocDefault));
    PRG_HIP(hipMemcpyAsync(h->L.pinned.p, h->state.p, count * sizeof(double), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < count; ++i) out_host[i] = h->L.pinned.p[i];
    return PRG_OK;
}

int prg_fr_get_state(prg_filterreg* h, double* out_host) {
    PRG_REQUIRE(h && out_host, PRG_ERR_INVALID, "prg_fr_get_state: NULL argument");
    PRG_ENTER(h->L.device);
    return fr_read_state(h, out_host, 20);
}

int prg_fr_mstep(prg_filterreg* h, double w, int update_sigma2, double min_sigma2, double* out_host) {
    PRG_REQUIRE(h && h->have_estep, PRG_ERR_STATE, "prg_fr_mstep: run prg_fr_estep first");
    PRG_REQUIRE(w >= 0.0 && w < 1.0, PRG_ERR_INVALID, "prg_fr_mstep: w must be in [0, 1) (got %g)", w);
    PRG_ENTER(h->L.device);
    hipStream_t st = h->L.stream;
    const double wfac = w / (1.0 - w) * (double)h->N / (double)h->M;
    const int nblk = (int)h->part_blocks;
    if (h->slice_pending) {  // slice + terms in one launch (the values still go to vout for prg_fr_get_estep)
        h->slice_pending = false;
        if (h->D == 2)
            k_fr_terms<true, true><<<nblk, kBlock, 0, st>>>(nullptr, h->vout.p, 5, h->L.pslot.p, h->L.bary.p, h->L.pend_vals,
                                                            h->L.pend_alpha, h->ts.p, h->M, h->D, wfac, h->state.p, h->part.p);
        else
            k_fr_terms<true><<<nblk, kBlock, 0, st>>>(nullptr, h->vout.p, 5, h->L.pslot.p, h->L.bary.p, h->L.pend_vals, h->L.pend_alpha,
                                                      h->ts.p, h->M, h->D, wfac, h->state.p, h->part.p);
    } else {
        k_fr_terms<false><<<nblk, kBlock, 0, st>>>(h->vout.p, nullptr, h->ch, nullptr, nullptr, nullptr, 0.f, h->ts.p, h->M, h->D, wfac,
                                                   h->state.p, h->part.p);
    }
    k_fr_finish<<<1, kBlock, 0, st>>>(h->part.p, nblk, h->D, update_sigma2, min_sigma2, h->state.p);
    PRG_HIP(hipGetLastError());
    return out_host ? fr_read_state(h, out_host, 18) : PRG_OK;  // NULL: nothing is read back, the stream keeps running
}

int prg_fr_set_target_normals(prg_filterreg* h, const double* normals_hd) {
    PRG_REQUIRE(h && h->have_tgt, PRG_ERR_STATE, "prg_fr_set_target_normals: target not set");
    PRG_REQUIRE(h->D == 3 || !normals_hd, PRG_ERR_INVALID, "prg_fr_set_target_normals: point-to-plane needs 3-D clouds");
    PRG_ENTER(h->L.device);
    PRG_HIP(hipStreamSynchronize(h->L.stream));
    h->have_estep = false;
    h->nrm.release();
    h->ch = 5;
    if (normals_hd) {
        PRG_HIP(h->nrm.reset(h->N * 3));
        std::vector<double> host((size_t)h->N * 3), sorted((size_t)h->N * 3);  // same order as the stored target
        PRG_HIP(hipMemcpy(host.data(), normals_hd, host.size() * sizeof(double), hipMemcpyDefault));
        for (int64_t i = 0; i < h->N; ++i)
            for (int k = 0; k < 3; ++k) sorted[(size_t)i * 3 + k] = host[(size_t)h->tgt_order[i] * 3 + k];
        PRG_HIP(hipMemcpyAsync(h->nrm.p, sorted.data(), (size_t)h->N * 3 * sizeof(double), hipMemcpyHostToDevice, h->L.stream));
        PRG_HIP(hipStreamSynchronize(h->L.stream));
        h->ch = 8;
    }
    return fr_alloc(h, &h->have_tgt);
}

int prg_fr_get_nx(prg_filterreg* h, float* nx_hd) {
    PRG_REQUIRE(h && h->have_estep && h->ch == 8 && nx_hd, PRG_ERR_STATE,
                "prg_fr_get_nx: needs target normals and an E-step");
    PRG_ENTER(h->L.device);
    return fr_fetch_columns(h, 5, 3, nx_hd);
}

int prg_fr_mstep_pt2pl(prg_filterreg* h, double w, int update_sigma2, double min_sigma2, double* out_host) {
    PRG_REQUIRE(h && h->have_estep, PRG_ERR_STATE, "prg_fr_mstep_pt2pl: run prg_fr_estep first");
    PRG_REQUIRE(h->ch == 8, PRG_ERR_STATE, "prg_fr_mstep_pt2pl: target normals have not been set");
    PRG_REQUIRE(w >= 0.0 && w < 1.0, PRG_ERR_INVALID, "prg_fr_mstep_pt2pl: w must be in [0, 1) (got %g)", w);
    PRG_ENTER(h->L.device);
    hipStream_t st = h->L.stream;
    const double wfac = w / (1.0 - w) * (double)h->N / (double)h->M;
    const int nblk = (int)h->part_blocks;
    PRG_TRY(fr_flush_slice(h));
    k_fr_terms_pt2pl<<<nblk, kBlock, 0, st>>>(h->vout.p, h->ts.p, h->M, wfac, h->state.p, h->part.p);
    k_fr_finish_pt2pl<<<1, kBlock, 0, st>>>(h->part.p, nblk, update_sigma2, min_sigma2, h->state.p);
    PRG_HIP(hipGetLastError());
    return out_host ? fr_read_state(h, out_host, 18) : PRG_OK;
}

// RigidFilterReg._maximization_step on explicit arrays (filterreg.py:158-196) - same kernels as prg_fr_mstep /
// prg_fr_mstep_pt2pl, fed from the caller's buffers instead of a plan's last E-step
int prg_fr_mstep_from_arrays(int device, void* hip_stream, const double* t_source_hd, int64_t m, int dim,
                             int64_t n_target, const float* m0_hd, const float* m1_hd, const float* m2_hd,
                             const float* nx_hd, const double* rot9, const double* t3, double sigma2, double w,
                             double* out_host) {
    PRG_REQUIRE(t_source_hd && m0_hd && m1_hd && rot9 && t3 && out_host, PRG_ERR_INVALID,
                "prg_fr_mstep_from_arrays: NULL argument");
    PRG_REQUIRE(m > 0 && n_target > 0 && (dim == 2 || dim == 3), PRG_ERR_INVALID,
                "prg_fr_mstep_from_arrays: need m > 0, n_target > 0 and dim in {2,3}");  // "dim must be 2 or 3", :161
    PRG_REQUIRE(!nx_hd || dim == 3, PRG_ERR_INVALID, "prg_fr_mstep_from_arrays: point-to-plane needs 3-D clouds");
    PRG_REQUIRE(w >= 0.0 && w < 1.0, PRG_ERR_INVALID, "prg_fr_mstep_from_arrays: w must be in [0, 1) (got %g)", w);
    PRG_REQUIRE(sigma2 > 0.0, PRG_ERR_INVALID, "prg_fr_mstep_from_arrays: sigma2 must be > 0 (got %g)", sigma2);
    PRG_ENTER(device);
    hipStream_t st = (hipStream_t)hip_stream;
    const int ch = nx_hd ? 8 : 5;
    const int nblk = (int)std::min<int64_t>(prg::ceil_div(m, kBlock), 512), npack = (int)prg::ceil_div(m, kBlock);
    DevBuf<char> b_in;
    DevBuf<double> b_ts, b_part, b_state;
    DevBuf<float> b_v;
    // staging: t_source | m0 | m1 | m2 | nx
    const size_t o_ts = 0, o_m0 = o_ts + (size_t)m * dim * sizeof(double), o_m1 = o_m0 + (size_t)m * sizeof(float),
                 o_m2 = o_m1 + (size_t)m * dim * sizeof(float), o_nx = o_m2 + (size_t)m * sizeof(float),
                 total = o_nx + (size_t)m * 3 * sizeof(float);
    PRG_HIP(b_in.reset((int64_t)total));
    PRG_HIP(b_ts.reset(m * 4));  // (x, y, z, 0) per point, as the terms kernels read it
    PRG_HIP(b_v.reset(m * ch));
    PRG_HIP(b_part.reset((int64_t)nblk * kFrComp));
    PRG_HIP(b_state.reset(64));
    char* in = b_in.p;
    PRG_HIP(hipMemcpyAsync(in + o_ts, t_source_hd, (size_t)m * dim * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(in + o_m0, m0_hd, (size_t)m * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(in + o_m1, m1_hd, (size_t)m * dim * sizeof(float), hipMemcpyDefault, st));
    if (m2_hd) PRG_HIP(hipMemcpyAsync(in + o_m2, m2_hd, (size_t)m * sizeof(float), hipMemcpyDefault, st));
    if (nx_hd) PRG_HIP(hipMemcpyAsync(in + o_nx, nx_hd, (size_t)m * 3 * sizeof(float), hipMemcpyDefault, st));
    double host_state[64] = {0.0};
    for (int i = 0; i < 9; ++i) host_state[i] = rot9[i];
    for (int i = 0; i < 3; ++i) host_state[9 + i] = t3[i];
    host_state[12] = sigma2;
    PRG_HIP(hipMemcpyAsync(b_state.p, host_state, sizeof(host_state), hipMemcpyHostToDevice, st));
    k_fr_pack_estep<<<npack, kBlock, 0, st>>>((const double*)(in + o_ts), (const float*)(in + o_m0),
                                             (const float*)(in + o_m1), m2_hd ? (const float*)(in + o_m2) : nullptr,
                                             nx_hd ? (const float*)(in + o_nx) : nullptr, m, dim, ch, b_ts.p, b_v.p);
    const double wfac = w / (1.0 - w) * (double)n_target / (double)m;
    const int update_sigma2 = m2_hd ? 1 : 0;
    if (nx_hd) {
        k_fr_terms_pt2pl<<<nblk, kBlock, 0, st>>>(b_v.p, b_ts.p, m, wfac, b_state.p, b_part.p);
        k_fr_finish_pt2pl<<<1, kBlock, 0, st>>>(b_part.p, nblk, update_sigma2, -1.0, b_state.p);
    } else {
        k_fr_terms<false><<<nblk, kBlock, 0, st>>>(b_v.p, nullptr, ch, nullptr, nullptr, nullptr, 0.f, b_ts.p, m, dim, wfac,
                                                   b_state.p, b_part.p);
        k_fr_finish<<<1, kBlock, 0, st>>>(b_part.p, nblk, dim, update_sigma2, -1.0, b_state.p);
    }
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(host_state, b_state.p, 18 * sizeof(double), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 18; ++i) out_host[i] = host_state[i];
    return PRG_OK;
}

// stand-alone weighted Kabsch (probreg/cc/kabsch.cc:6-109 behind _kabsch.kabsch / kabsch2d)
int prg_kabsch_weighted(int device, void* hip_stream, const float* model_hd, const float* target_hd,
                        const float* weight_hd, int64_t n, int dim, double* rot_host, double* t_host) {
    PRG_REQUIRE(model_hd && target_hd && weight_hd && rot_host && t_host, PRG_ERR_INVALID,
                "prg_kabsch_weighted: NULL argument");
    PRG_REQUIRE(n > 0 && (dim == 2 || dim == 3), PRG_ERR_INVALID, "prg_kabsch_weighted: need n > 0, dim in {2,3}");
    PRG_ENTER(device);
    hipStream_t st = (hipStream_t)hip_stream;
    const int nblk = (int)prg::ceil_div(n, kBlock);
    DevBuf<float> bm, bt, bw;
    DevBuf<double> bp, bo;
    PRG_HIP(bm.reset(n * dim));
    PRG_HIP(bt.reset(n * dim));
    PRG_HIP(bw.reset(n));
    PRG_HIP(bp.reset((int64_t)nblk * kFrComp));
    PRG_HIP(bo.reset(12));
    PRG_HIP(hipMemcpyAsync(bm.p, model_hd, (size_t)n * dim * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(bt.p, target_hd, (size_t)n * dim * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(bw.p, weight_hd, (size_t)n * sizeof(float), hipMemcpyDefault, st));
    k_kabsch_terms<<<nblk, kBlock, 0, st>>>(bm.p, bt.p, bw.p, n, dim, bp.p);
    k_kabsch_finish<<<1, kBlock, 0, st>>>(bp.p, nblk, dim, bo.p);
    PRG_HIP(hipGetLastError());
    double out[12];
    PRG_HIP(hipMemcpyAsync(out, bo.p, sizeof(out), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < dim; ++i) {
        t_host[i] = out[9 + i];
        for (int j = 0; j < dim; ++j) rot_host[i * dim + j] = out[3 * i + j];
    }
    return PRG_OK;
}

}  // extern "C"
