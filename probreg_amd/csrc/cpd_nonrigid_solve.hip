// Non-rigid CPD M-step on MI355X (gfx950): dense fp64 solve on the f64 matrix cores.
//
// Reference (neka-nat/probreg v0.3.7, probreg/cpd.py:284-303):
//     W = solve(diag(p1) G + lmd*sigma2_prev*I,  px - diag(p1) Y)        (LAPACK gesv, float64)
//     T = Y + G W ;  sigma2 = (tr(X^T diag(pt1) X) - 2 tr(px^T T) + tr(T^T diag(p1) T)) / (n_p D)
//
// The system matrix A = D G + c I (D = diag(p1), c = lmd*sigma2_prev) is not symmetric, but with
// U = D^1/2 and V = D^1/2 G the push-through identity
//     (c I + U V)^-1 = (1/c) (I - U (c I + V U)^-1 V)
// turns it into one SPD system in S = c I + D^1/2 G D^1/2 (eigenvalues >= c > 0, legal for p1 >= 0):
//     W = (B - D^1/2 S^-1 D^1/2 (G B)) / c ,   B = px - D Y.
// S is factored, and the systems solved, by the blocked fp64 Cholesky of spd_solve.hip (cond(S) reaches 1e7-1e8: c ~ 1e-3,
// lambda_max(G) ~ M); the workspace is carved by cpd_solve_layout.h.  The BCPD solve on the same parts: cpd_bcpd_solve.hip.
//
// Tests that hold each path to round-off level (8 x the disagreement of two float64 host solves; tests/test_dense_solve_gpu.py):
//   dense M-step, every class of the look-ahead schedule     test_dense_mstep_per_schedule_class, test_rows_without_support
//   correspondence priors and their two refinement steps      test_constrained_mstep_dense, test_constrained_mstep_lowrank
//   non-positive pivots: immediate report / sticky flag       test_dense_path_reports_..., test_lowrank_path_reports_...
//   low-rank M-step                                           tests/test_nonrigid_lowrank_gpu.py (1e-7 on the exact matrix)
#include <math.h>

#include <algorithm>

#include "cpd_solve_drivers.h"
#include "prg_device.h"

namespace {
constexpr int kBlock = prg::kSolveThreads;
constexpr int NB = prg::kSpdBlock;
typedef double d4 __attribute__((ext_vector_type(4)));
}  // namespace

// ---- kernels the BCPD solve launches too (declared in cpd_solve_drivers.h) -----------------------------------------------
namespace prg {
// S = c I + diag(sp) G diag(sp) on the lower 128-tiles (diagonal tiles full); identity in the pad.
__global__ __launch_bounds__(kBlock) void k_build_s(const float* __restrict__ g, int64_t m, int64_t mp,
                                                    const double* __restrict__ sp, const double* __restrict__ params,
                                                    double lmd, double* __restrict__ s) {
    const int by = blockIdx.y, bx = blockIdx.x;
    if (bx > by) return;
    const double c = params ? lmd * params[13] : lmd;  // params == nullptr: lmd carries c itself (BCPD)
    const int tx = threadIdx.x & 127, ty = threadIdx.x >> 7;  // 128 columns x 2 rows per pass
    const int64_t j = (int64_t)bx * NB + tx;
    const double spj = j < m ? sp[j] : 0.0;
    for (int r = ty; r < NB; r += 2) {
        const int64_t i = (int64_t)by * NB + r;
        double v;
        if (i < m && j < m)
            v = sp[i] * (double)g[i * m + j] * spj + (i == j ? c : 0.0);
        else
            v = (i == j) ? 1.0 : 0.0;
        s[i * mp + j] = v;
    }
}

// v = sp .* gb
__global__ __launch_bounds__(kBlock) void k_scale_rows(const double* __restrict__ sp, const double* __restrict__ in,
                                                       int64_t mp, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp) return;
    const double f = sp[i];
    out[i * 3] = f * in[i * 3];
    out[i * 3 + 1] = f * in[i * 3 + 1];
    out[i * 3 + 2] = f * in[i * 3 + 2];
}
}  // namespace prg

namespace {

// ---- right-hand side ----------------------------------------------------------------------------
// B = px - p1 * y   (cpd.py:296, right-hand side), rows >= m zero.  sp = sqrt(p1).
// With correspondence priors (ConstrainedNonRigidCPD, cpd.py:391-396): p1 -> p1 + sigma2/alpha * p1_tilde on the
// left-hand side and B += sigma2/alpha * (px_tilde - p1_tilde * y).
__global__ __launch_bounds__(kBlock) void k_rhs(const double* __restrict__ rowacc, int64_t mcap,
                                                const float4* __restrict__ src4, int64_t m, int64_t mp,
                                                const double* __restrict__ prior, double alpha,
                                                const double* __restrict__ params, double* __restrict__ b3,
                                                double* __restrict__ sp) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp) return;
    if (i < m) {
        double p1 = rowacc[i];
        const float4 y = src4[i];
        double b0 = rowacc[mcap + i] - p1 * (double)y.x;
        double b1 = rowacc[2 * mcap + i] - p1 * (double)y.y;
        double b2 = rowacc[3 * mcap + i] - p1 * (double)y.z;
        if (prior) {
            const double f = params[13] / alpha, pt = prior[i];
            b0 += f * (prior[m + i] - pt * (double)y.x);
            b1 += f * (prior[2 * m + i] - pt * (double)y.y);
            b2 += f * (prior[3 * m + i] - pt * (double)y.z);
            p1 += f * pt;
        }
        b3[i * 3 + 0] = b0;
        b3[i * 3 + 1] = b1;
        b3[i * 3 + 2] = b2;
        sp[i] = sqrt(fmax(p1, 0.0));
    } else {
        b3[i * 3] = b3[i * 3 + 1] = b3[i * 3 + 2] = 0.0;
        sp[i] = 0.0;
    }
}

// w = (b - sp .* u) / c
__global__ __launch_bounds__(kBlock) void k_form_w(const double* __restrict__ b3, const double* __restrict__ sp,
                                                   const double* __restrict__ u, int64_t m,
                                                   const double* __restrict__ params, double lmd,
                                                   double* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const double rc = 1.0 / (lmd * params[13]);
    const double f = sp[i];
    w[i * 3] = (b3[i * 3] - f * u[i * 3]) * rc;
    w[i * 3 + 1] = (b3[i * 3 + 1] - f * u[i * 3 + 1]) * rc;
    w[i * 3 + 2] = (b3[i * 3 + 2] - f * u[i * 3 + 2]) * rc;
}

// iterative refinement: r = b - (sp^2 .* (G w) + c w)   (residual of (D G + c I) w = b, fp64)
__global__ __launch_bounds__(kBlock) void k_residual(const double* __restrict__ b3, const double* __restrict__ sp,
                                                     const double* __restrict__ gw, const double* __restrict__ w,
                                                     int64_t m, int64_t mp, const double* __restrict__ params,
                                                     double lmd, double* __restrict__ r3) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp) return;
    if (i < m) {
        const double c = lmd * params[13], d = sp[i] * sp[i];
        for (int k = 0; k < 3; ++k) r3[i * 3 + k] = b3[i * 3 + k] - (d * gw[i * 3 + k] + c * w[i * 3 + k]);
    } else {
        r3[i * 3] = r3[i * 3 + 1] = r3[i * 3 + 2] = 0.0;
    }
}
__global__ __launch_bounds__(kBlock) void k_axpy3(const double* __restrict__ x, int64_t m, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < m * 3) y[i] += x[i];
}

// partial sums of tr(px^T T) and tr(T^T diag(p1) T), T = y + gw   (cpd.py:298-300)
__global__ __launch_bounds__(kBlock) void k_traces(const double* __restrict__ rowacc, int64_t mcap,
                                                   const float4* __restrict__ src4, const double* __restrict__ gw,
                                                   int64_t m, double* __restrict__ part) {
    __shared__ double sh[4][2];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double a = 0.0, b = 0.0;
    if (i < m) {
        const float4 y = src4[i];
        const double t0 = (double)y.x + gw[i * 3], t1 = (double)y.y + gw[i * 3 + 1], t2 = (double)y.z + gw[i * 3 + 2];
        a = rowacc[mcap + i] * t0 + rowacc[2 * mcap + i] * t1 + rowacc[3 * mcap + i] * t2;
        b = rowacc[i] * (t0 * t0 + t1 * t1 + t2 * t2);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) { sh[wv][0] = a; sh[wv][1] = b; }
    __syncthreads();
    if (threadIdx.x < 2)
        part[(int64_t)blockIdx.x * 2 + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] +
                                                     sh[3][threadIdx.x];
}

__global__ void k_nonrigid_finish(const double* __restrict__ part, int nblk, const double* __restrict__ mom,
                                  double* __restrict__ params, int dim) {
    __shared__ double sh[2][64];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) {
        a += part[2 * i];
        b += part[2 * i + 1];
    }
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tr_pxt = 0.0, tr_tpt = 0.0;
        for (int i = 0; i < 64; ++i) { tr_pxt += sh[0][i]; tr_tpt += sh[1][i]; }
        const double n_p = mom[0], tr_xp1x = mom[22];
        const double sigma2 = (tr_xp1x - 2.0 * tr_pxt + tr_tpt) / (n_p * dim);  // cpd.py:301 (no eps clamp)
        params[13] = sigma2;
        params[14] = sigma2;  // q := sigma2, cpd.py:303
        params[15] = n_p;
        params[16] += 1.0;
    }
}

// ---- low-rank M-step (G = F F^T, cpd_nonrigid.hip) ---------------------------------------------------------------
// (D G + c I) W = B with G = F F^T:   W = (B - D F Z) / c,   (c I + F^T D F) Z = F^T B     (push-through identity again,
// now with an r x r SPD system, r = rank of the factor: M r^2 flop instead of M^3 / 3 and no M x M matrix at all).
// T = F^T D F on 64 x 64 tiles of the lower triangle; the sum over the points is split over workgroups, each of which
// writes its partial tile; k_lr_gram_reduce adds them up in a fixed order (reproducible) and puts c on the diagonal.
constexpr int GT = prg::kGramTile;  // tile edge
constexpr int GS = prg::kGramSlab;  // points per LDS slab
constexpr int GLD = GT + 1;
}  // namespace

namespace prg {  // (k_lr_gram, k_lr_gram_reduce: launched by the BCPD solve too)
// The tile products run on the f64 matrix cores (v_mfma_f64_16x16x4_f64: wave w owns the 32 x 32 quadrant (w >> 1, w & 1)
// as 2 x 2 MFMA tiles, operands from the LDS slab).  Workgroups of the first tile column (tb == 0) also form their rows of
// u = F^T B with one more MFMA per k-step (B = [b | 0] as a 16-column operand), so the right-hand side of the reduced
// system costs no pass of its own.
__global__ __launch_bounds__(kBlock) void k_lr_gram(const double* __restrict__ f, int64_t ld, int64_t m, int rank,
                                                    const double* __restrict__ sp, const double* __restrict__ dw,
                                                    const double* __restrict__ b3, int64_t chunk,
                                                    double* __restrict__ part, double* __restrict__ upart) {
    __shared__ double as[GS][GLD], bs[GS][GLD], xs[GS][16];
    // tile (ta >= tb) of the lower triangle from the linear index
    int ta = 0, rem = blockIdx.x;
    while (rem > ta) {
        rem -= ta + 1;
        ++ta;
    }
    const int tb = rem;
    const int a0 = ta * GT, b0 = tb * GT;
    const int64_t i_begin = (int64_t)blockIdx.y * chunk, i_end = i_begin + chunk < m ? i_begin + chunk : m;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = wv >> 1, wc = wv & 1, li = lane & 15, kq = lane >> 4;
    const int lk = threadIdx.x & 31, lr = threadIdx.x >> 5;  // staging: point lk of the slab, factor rows lr + 8 q
    const bool with_u = tb == 0;
    d4 acc[2][2], uacc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        uacc[i] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    }
    (&xs[0][0])[threadIdx.x] = 0.0;  // columns 3..15 of the right-hand-side operand stay zero
    (&xs[0][0])[threadIdx.x + kBlock] = 0.0;
    // software pipeline: the global loads of slab t + 1 are in flight while the matrix cores work on slab t (all loads of
    // a slab are issued before the first LDS store - interleaved, every store would wait for its own load's round trip)
    double ra[GT / 8], rb[GT / 8], rx = 0.0;
    auto fetch = [&](int64_t i0) {
        const int64_t i = i0 + lk;
        const bool in = i < i_end;
        // D_ii: k_rhs left sqrt(D) in sp; the BCPD M-step passes nu itself in dw (sqrt(nu)^2 is an ulp off)
        const double pw = in ? (dw ? dw[i] : sp[i] * sp[i]) : 0.0;
#pragma unroll
        for (int q = 0; q < GT / 8; ++q) {
            const int r = lr + 8 * q;
            ra[q] = (in && a0 + r < rank) ? f[(int64_t)(a0 + r) * ld + i] : 0.0;
            rb[q] = (in && b0 + r < rank) ? f[(int64_t)(b0 + r) * ld + i] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < GT / 8; ++q) rb[q] *= pw;
        if (with_u && lr < 3) rx = in ? b3[i * 3 + lr] : 0.0;
    };
    fetch(i_begin);
    for (int64_t i0 = i_begin; i0 < i_end; i0 += GS) {
        __syncthreads();  // the previous slab has been consumed
#pragma unroll
        for (int q = 0; q < GT / 8; ++q) {
            as[lk][lr + 8 * q] = ra[q];
            bs[lk][lr + 8 * q] = rb[q];
        }
        if (with_u && lr < 3) xs[lk][lr] = rx;
        __syncthreads();
        if (i0 + GS < i_end) fetch(i0 + GS);
#pragma unroll
        for (int k4 = 0; k4 < GS; k4 += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                av[t] = as[k4 + kq][wr * 32 + 16 * t + li];
                bv[t] = bs[k4 + kq][wc * 32 + 16 * t + li];
            }
#pragma unroll
            for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
                for (int j2 = 0; j2 < 2; ++j2)
                    acc[i2][j2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i2], bv[j2], acc[i2][j2], 0, 0, 0);
            if (with_u && wc == 0) {
                const double xv = xs[k4 + kq][li];
                uacc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[0], xv, uacc[0], 0, 0, 0);
                uacc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[1], xv, uacc[1], 0, 0, 0);
            }
        }
    }
    // C/D map of the MFMA: row = (lane >> 4) + 4 reg, column = lane & 15
    double* __restrict__ out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (GT * GT);
#pragma unroll
    for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(wr * 32 + 16 * i2 + kq + 4 * r) * GT + wc * 32 + 16 * j2 + li] = acc[i2][j2][r];
    if (with_u && wc == 0 && li < 3) {  // upart[split][row][3]
        double* __restrict__ uo = upart + (int64_t)blockIdx.y * ((int64_t)rank * 3);
#pragma unroll
        for (int i2 = 0; i2 < 2; ++i2)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = a0 + wr * 32 + 16 * i2 + kq + 4 * r;
                if (row < rank) uo[(int64_t)row * 3 + li] = uacc[i2][r];
            }
    }
}

// S[a][b] = c [a == b] + sum over the splits of T's tile entry (a, b) for a, b < rank; identity in the pad (rp x rp).
// Four lanes share an output element: each sums every fourth split, the four partial sums are combined in a fixed order
// (reproducible; the loads of the four chains run in parallel - one thread walking all splits is a chain of dependent adds
// behind ~80 loads).
__global__ __launch_bounds__(kBlock) void k_lr_gram_reduce(const double* __restrict__ part, const double* __restrict__ upart,
                                                           int ntile, int nsplit, int rank, int64_t rp,
                                                           const double* __restrict__ params, double lmd,
                                                           double* __restrict__ s, double* __restrict__ u) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t e = t >> 2;
    const int sub = (int)(t & 3);
    double v = 0.0, uv = 0.0;
    const bool in_u = e < (int64_t)rank * 3;
    const int a = (int)(e / rp), b = (int)(e % rp);
    const bool in_s = e < rp * rp, real = in_s && a < rank && b < rank;
    if (in_u) {  // u = F^T B
        const double* __restrict__ src = upart + e;
        const int64_t st = (int64_t)rank * 3;
        for (int q = sub; q < nsplit; q += 4) uv += src[q * st];
    }
    if (real) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;  // lower triangle holds (hi, lo)
        const int ta = hi / GT, tb = lo / GT;
        const int tile = ta * (ta + 1) / 2 + tb;
        const int r = hi - ta * GT, c = lo - tb * GT;
        const double* __restrict__ src = part + (int64_t)tile * (GT * GT) + r * GT + c;
        const int64_t st = (int64_t)ntile * (GT * GT);
        for (int q = sub; q < nsplit; q += 4) v += src[q * st];
    }
    // (lanes 4k .. 4k+3 hold the four chains of one element)
    v = (v + __shfl_xor(v, 1, 64));
    v = (v + __shfl_xor(v, 2, 64));
    uv = (uv + __shfl_xor(uv, 1, 64));
    uv = (uv + __shfl_xor(uv, 2, 64));
    if (sub != 0) return;
    if (e < rp * 3) u[e] = in_u ? uv : 0.0;  // zero rows in the pad
    if (!in_s) return;
    if (real) {
        if (a == b) v += params ? lmd * params[13] : lmd;  // params == nullptr: lmd carries the shift itself (BCPD)
    } else {
        v = a == b ? 1.0 : 0.0;
    }
    s[e] = v;
}

int ensure_solve_workspace(prg_cpd* h, size_t need, bool lowrank) {
    const bool fresh = h->nr_solve.cap < (int64_t)need;
    if (fresh) {
        if (h->nr_solve.p) PRG_HIP(hipStreamSynchronize(h->stream));
        h->nr_info = nullptr;
        PRG_HIP(h->nr_solve.reset((int64_t)need));
        if (lowrank) PRG_HIP(hipMemsetAsync(h->nr_solve.p, 0, need * sizeof(double), h->stream));
    }
    h->nr_queues.main = h->stream;
    // the solver's LDS opt-in: the low-rank solves ask on every call, as they always have, the dense ones with a new block
    if (lowrank || fresh) PRG_TRY(spd_prepare());
    return PRG_OK;
}

int report_pivot(prg_cpd* h, const int* info, const char* who, const char* hint) {
    int host_info = 0;
    PRG_HIP(hipMemcpyAsync(&host_info, info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_REQUIRE(host_info == 0, PRG_ERR_STATE, "%s: S is not positive definite at pivot %d%s", who, host_info - 1, hint);
    return PRG_OK;
}
}  // namespace prg

namespace {
using prg::solve_grid1;

// w = (b - D F z) / c
__global__ __launch_bounds__(kBlock) void k_lr_form_w(const double* __restrict__ b3, const double* __restrict__ sp,
                                                      const double* __restrict__ fz, int64_t m,
                                                      const double* __restrict__ params, double lmd,
                                                      double* __restrict__ w) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const double rc = 1.0 / (lmd * params[13]);
    const double d = sp[i] * sp[i];
    w[i * 3] = (b3[i * 3] - d * fz[i * 3]) * rc;
    w[i * 3 + 1] = (b3[i * 3 + 1] - d * fz[i * 3 + 1]) * rc;
    w[i * 3 + 2] = (b3[i * 3 + 2] - d * fz[i * 3 + 2]) * rc;
}

int mstep_nonrigid_lowrank(prg_cpd* h, double lmd) {
    const int64_t m = h->M, ld = h->f_ld;
    const int rank = h->f_rank;
    const prg::LowRankLayout L = prg::make_lowrank_layout(m, ld, rank);
    const prg::NonrigidLowrankWs o = prg::nonrigid_lowrank_ws(L, m);
    const int64_t rp = L.rp;
    const int tr_blk = (int)prg::ceil_div(m, kBlock);
    PRG_TRY(prg::ensure_solve_workspace(h, o.total, true));
    double* const ws = h->nr_solve.p;
    double *S = ws + o.S, *part = ws + o.part, *upart = ws + o.upart, *b3 = ws + o.b3, *sp = ws + o.sp, *fz = ws + o.fz,
           *gb = ws + o.gb, *r3 = ws + o.r3, *dw = ws + o.dw, *z = ws + o.z, *trpart = ws + o.trpart;
    int* info = reinterpret_cast<int*>(ws + o.info);
    const prg::SpdFactor fac{S, ws + o.linv, rp, rank, L.small};
    hipStream_t st = h->stream;
    const dim3 ggrid((unsigned)L.ntile, (unsigned)L.nsplit);
    const dim3 rgrid = solve_grid1(4 * std::max<int64_t>((int64_t)rp * rp, rp * 3));  // four lanes per element

    // (info is sticky: cleared when the workspace is allocated and when prg_cpd_get_params has reported it)
    k_rhs<<<solve_grid1(ld), kBlock, 0, st>>>(h->rowacc.p, h->Mcap, h->src4.p, m, ld, h->nr_alpha > 0.0 ? h->nr_prior.p : nullptr,
                                              h->nr_alpha, h->params, b3, sp);
    // S = c I + F^T D F and z = F^T B in one pass over the factor
    prg::k_lr_gram<<<ggrid, kBlock, 0, st>>>(h->F.p, ld, m, rank, sp, nullptr, b3, L.chunk, part, upart);
    prg::k_lr_gram_reduce<<<rgrid, kBlock, 0, st>>>(part, upart, L.ntile, L.nsplit, rank, rp, h->params, lmd, S, z);
    // (one workgroup doing the whole r x r solve out of LDS was built in round 3: with the packed triangle's irregular LDS
    // addressing it took 270 us at r = 176, more than the ten launches of the small factorisation - 240 us - and was removed)
    PRG_TRY(prg::spd_factor(h->nr_queues, fac, info));
    PRG_TRY(prg::spd_solve3(h->nr_queues, fac, z));  // z = (c I + F^T D F)^-1 F^T B
    double* gw = h->nr_work.p;                      // [M][3]: G W, kept for the next E-step's transform
    // W = (B - D F z) / c ... and G W = F (F^T W) = F z exactly: F^T W = (F^T B - F^T D F z) / c = (S z - (S - c I) z) / c
    PRG_TRY(prg::lowrank_apply(h, z, gw));
    k_lr_form_w<<<solve_grid1(m), kBlock, 0, st>>>(b3, sp, gw, m, h->params, lmd, h->W.p);
    // With correspondence priors the diagonal scaling spans sigma2/alpha ~ 1e7 and the push-through form loses digits
    // to cancellation: two steps of fp64 iterative refinement on the original system (see prg_cpd_mstep_nonrigid)
    const int nrefine = h->nr_alpha > 0.0 ? 2 : 0;
    for (int it = 0; it < nrefine; ++it) {
        PRG_TRY(prg::nonrigid_gw(h, h->W.p, gb));
        k_residual<<<solve_grid1(ld), kBlock, 0, st>>>(b3, sp, gb, h->W.p, m, ld, h->params, lmd, r3);
        if (rp > rank) PRG_HIP(hipMemsetAsync(z + (size_t)rank * 3, 0, (size_t)(rp - rank) * 3 * sizeof(double), st));
        PRG_TRY(prg::lowrank_ft3(h, r3, z));
        PRG_TRY(prg::spd_solve3(h->nr_queues, fac, z));
        PRG_TRY(prg::lowrank_apply(h, z, fz));
        k_lr_form_w<<<solve_grid1(m), kBlock, 0, st>>>(r3, sp, fz, m, h->params, lmd, dw);
        k_axpy3<<<solve_grid1(m * 3), kBlock, 0, st>>>(dw, m, h->W.p);
    }
    if (nrefine > 0) PRG_TRY(prg::nonrigid_gw(h, h->W.p, gw));
    k_traces<<<tr_blk, kBlock, 0, st>>>(h->rowacc.p, h->Mcap, h->src4.p, gw, m, trpart);
    k_nonrigid_finish<<<1, 64, 0, st>>>(trpart, tr_blk, h->moments, h->params, h->D);
    PRG_HIP(hipGetLastError());
    h->gw_valid = true;
    // The pivot check does not stall the stream: the flag is looked at the next time the host synchronises anyway
    // (prg_cpd_get_params / the next M-step), where a failure of this step is reported.
    h->nr_info = info;
    return PRG_OK;
}

}  // namespace

extern "C" int prg_cpd_mstep_nonrigid(prg_cpd* h, double lmd) {
    PRG_REQUIRE(h && (h->G.p || h->F.p) && h->W.p && h->have_estep, PRG_ERR_STATE,
                "prg_cpd_mstep_nonrigid: needs build_g and an E-step first");
    PRG_REQUIRE(lmd > 0.0, PRG_ERR_INVALID, "prg_cpd_mstep_nonrigid: lmd must be > 0 (got %g)", lmd);
    PRG_ENTER(h->device);
    h->estep_state_live = false;  // sigma2 in PARAMS is the next E-step's now
    if (h->F.p) return mstep_nonrigid_lowrank(h, lmd);
    const int64_t m = h->M, mp = prg::round_up(m, NB), nblk = mp / NB;
    // workspace: S [mp*mp] | Linv [nblk*128*128] | b3, gb, v, sp, r3, dw (each 3 mp) | trace partials | info
    const prg::NonrigidDenseWs o = prg::nonrigid_dense_ws(m);
    const int tr_blk = (int)prg::ceil_div(m, kBlock);
    PRG_TRY(prg::ensure_solve_workspace(h, o.total, false));
    double* const ws = h->nr_solve.p;
    double *S = ws + o.S, *b3 = ws + o.b3, *gb = ws + o.gb, *v = ws + o.v, *sp = ws + o.sp, *r3 = ws + o.r3, *dw = ws + o.dw,
           *trpart = ws + o.trpart;
    int* info = reinterpret_cast<int*>(ws + o.info);
    const prg::SpdFactor fac{S, ws + o.linv, mp, m, false};
    hipStream_t st = h->stream;

    PRG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
    k_rhs<<<solve_grid1(mp), kBlock, 0, st>>>(h->rowacc.p, h->Mcap, h->src4.p, m, mp, h->nr_alpha > 0.0 ? h->nr_prior.p : nullptr,
                                              h->nr_alpha, h->params, b3, sp);
    prg::k_build_s<<<dim3((unsigned)nblk, (unsigned)nblk), kBlock, 0, st>>>(h->G.p, m, mp, sp, h->params, lmd, S);

    PRG_TRY(prg::spd_factor(h->nr_queues, fac, info));
    // w = (rhs - D^1/2 S^-1 D^1/2 (G rhs)) / c with the factor above: two blocked triangular sweeps, 3 RHS
    auto solve_with_factor = [&](const double* rhs, double* wout) -> int {
        PRG_TRY(prg::nonrigid_gw(h, rhs, gb));                               // G rhs
        prg::k_scale_rows<<<solve_grid1(m), kBlock, 0, st>>>(sp, gb, m, v);  // v = D^1/2 G rhs
        if (mp > m) PRG_HIP(hipMemsetAsync(v + m * 3, 0, (size_t)(mp - m) * 3 * sizeof(double), st));
        PRG_TRY(prg::spd_solve3(h->nr_queues, fac, v));
        k_form_w<<<solve_grid1(m), kBlock, 0, st>>>(rhs, sp, v, m, h->params, lmd, wout);
        PRG_HIP(hipGetLastError());
        return PRG_OK;
    };
    PRG_TRY(solve_with_factor(b3, h->W.p));
    // With correspondence priors the diagonal scaling spans sigma2/alpha ~ 1e7 and the push-through form
    // loses digits to cancellation; two steps of fp64 iterative refinement on the ORIGINAL system
    // (D G + c I) w = b bring the solution back to the backward-stable level LAPACK gesv delivers.
    const int nrefine = h->nr_alpha > 0.0 ? 2 : 0;
    for (int it = 0; it < nrefine; ++it) {
        PRG_TRY(prg::nonrigid_gw(h, h->W.p, gb));
        k_residual<<<solve_grid1(mp), kBlock, 0, st>>>(b3, sp, gb, h->W.p, m, mp, h->params, lmd, r3);
        PRG_TRY(solve_with_factor(r3, dw));
        k_axpy3<<<solve_grid1(m * 3), kBlock, 0, st>>>(dw, m, h->W.p);
    }
    PRG_TRY(prg::nonrigid_gw(h, h->W.p, h->nr_work.p));            // G W, kept for the next E-step's transform
    k_traces<<<tr_blk, kBlock, 0, st>>>(h->rowacc.p, h->Mcap, h->src4.p, h->nr_work.p, m, trpart);
    k_nonrigid_finish<<<1, 64, 0, st>>>(trpart, tr_blk, h->moments, h->params, h->D);
    PRG_HIP(hipGetLastError());
    h->gw_valid = true;
    return prg::report_pivot(h, info, "prg_cpd_mstep_nonrigid", " (sigma2 or lmd <= 0?)");
}
