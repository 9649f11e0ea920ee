// BCPD solve on MI355X (gfx950): prg_cpd_bcpd_solve, dense and on the kernel factor, on the blocked fp64 Cholesky of
// spd_solve.hip.  The kernels it shares with the non-rigid M-step are cpd_nonrigid_solve.hip's (cpd_solve_drivers.h).
//
// Tests that hold each path to round-off level:
//   dense (K-deep left update, second panel), its pivot report   tests/test_dense_solve_gpu.py::test_bcpd_solve, test_bcpd_gpu.py
//   on the kernel factor, diag(Sigma)                             tests/test_bcpd_lowrank_gpu.py::test_solve_on_the_factor
//
// BCPD M-step core (reference bcpd.py:123-133): with nu = row sums of P, c = s^2 / sigma2_prev^2,
//     Sigma = (lmd G^-1 + c diag(nu))^-1,   v_hat = c Sigma diag(nu) R,   R = T^-1(x_hat) - y.
// The reference inverts G and then the M x M sum explicitly.  Here G^-1 never appears: by Woodbury, with
// D = diag(nu) and the SPD matrix S = (lmd / c) I + D^1/2 G D^1/2 = L L^T,
//     Sigma = (G - B^T S^-1 B) / lmd,   B = D^1/2 G,
// so  diag(Sigma)_m = (g_mm - |L^-1 B e_m|^2) / lmd   (a triangular solve with M right-hand sides, on the
// matrix cores, M^3 flop) and  v_hat = (c / lmd) (G b - B^T S^-1 B b),  b = D R  (3 right-hand sides).
// The form stays finite for nu_m -> 0 (points without support), where Sigma_mm -> g_mm / lmd.
#include <math.h>

#include <algorithm>

#include "cpd_solve_drivers.h"
#include "prg_device.h"

namespace {

constexpr int kBlock = prg::kSolveThreads;
constexpr int NB = prg::kSpdBlock;
typedef double d4 __attribute__((ext_vector_type(4)));
using prg::solve_grid1;

__global__ __launch_bounds__(kBlock) void k_bcpd_rhs(const double* __restrict__ rowacc, const double* __restrict__ nu_ext,
                                                     const double* __restrict__ resid, const int* __restrict__ perm,
                                                     int64_t m, int64_t mp, int dim, double* __restrict__ b3,
                                                     double* __restrict__ sp, double* __restrict__ nu_out = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= mp) return;
    double nu = 0.0, r[3] = {0.0, 0.0, 0.0};
    if (i < m) {
        const int64_t j = perm ? perm[i] : i;
        nu = fmax(nu_ext ? nu_ext[j] : rowacc[i], 0.0);  // nu_ext is in the caller's order, rowacc in kernel order
        for (int k = 0; k < dim; ++k) r[k] = resid[j * dim + k];
    }
    b3[i * 3] = nu * r[0];
    b3[i * 3 + 1] = nu * r[1];
    b3[i * 3 + 2] = nu * r[2];
    sp[i] = sqrt(nu);
    if (nu_out) nu_out[i] = nu;
}

// Wt[c][j] = g[c][j] * sp[j]  (= (D^1/2 G)^T, G symmetric); zero in the pad
__global__ __launch_bounds__(kBlock) void k_build_bt(const float* __restrict__ g, int64_t m, int64_t mp,
                                                     const double* __restrict__ sp, double* __restrict__ wt) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= mp) return;
    const double spj = j < m ? sp[j] : 0.0;
    for (int64_t c = blockIdx.y; c < mp; c += gridDim.y)
        wt[c * mp + j] = (c < m && j < m) ? (double)g[c * m + j] * spj : 0.0;
}

// diag[i] = (g_ii - sum_j Wt[i][j]^2) / lmd ; one wave per row
__global__ __launch_bounds__(kBlock) void k_sigma_diag(const double* __restrict__ wt, const float* __restrict__ g,
                                                       int64_t m, int64_t mp, double lmd, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const double* row = wt + i * mp;
    double a = 0.0;
    for (int64_t j = lane * 2; j < mp; j += 128) {
        const double2 v = *reinterpret_cast<const double2*>(row + j);
        a += v.x * v.x + v.y * v.y;
    }
    a = wave_sum(a);
    if (lane == 0) out[i] = ((double)g[i * m + i] - a) / lmd;
}

__global__ __launch_bounds__(kBlock) void k_bcpd_vhat(const double* __restrict__ gb, const double* __restrict__ gt,
                                                      int64_t m, double f, double* __restrict__ v) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < m * 3) v[i] = f * (gb[i] - gt[i]);
}

__global__ __launch_bounds__(kBlock) void k_unsort_rows(const double* __restrict__ in, int stride_in, int dim,
                                                        int64_t m, const int* __restrict__ perm,
                                                        double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int64_t j = perm ? perm[i] : i;
    for (int k = 0; k < dim; ++k) out[j * dim + k] = in[i * stride_in + k];
}

// ---- BCPD M-step on the kernel factor G = F F^T -------------------------------------------------------
// With D = diag(nu), c = cfac and the r x r SPD matrix S = (lmd / c) I + F^T D F = L L^T (push-through identity: no G^-1 and
// no division by nu, so nu_m = 0 is no special case):
//     Sigma = (lmd G^-1 + c D)^-1 = (1 / c) F S^-1 F^T,    v_hat = c Sigma D R = F S^-1 (F^T D R),
//     Sigma_mm = |L^-1 f_m|^2 / c                           (f_m = row m of F; a sum of squares, never negative).
// S comes from k_lr_gram (which also forms F^T D R), the r x r Cholesky and the three-right-hand-side solves are the
// low-rank non-rigid M-step's; new here is diag(Sigma): M r^2 flop, the only part whose cost grows with M r^2.

// X = L^-1 (lower triangular, [rp][rp] row-major; the upper triangle and every row / column >= rank are written as zeros)
// from the Cholesky factor in the lower triangle of s.  The columns of X are independent forward substitutions
// L x = e_c: one workgroup per strip of 16 columns, walking down 16 rows at a time - the products with the rows
// already finished are one dot product per thread (fixed order), the 16 x 16 diagonal block is substituted out of LDS.
// (x is read back by the workgroup that wrote it, after a barrier: no __restrict__.)
constexpr int TI = 16;
__global__ __launch_bounds__(kBlock) void k_tri_inverse(const double* __restrict__ s, int64_t rp, int rank, double* x) {
    __shared__ double lblk[TI][TI + 1], xb[TI][TI + 1];
    const int c0 = blockIdx.x * TI;
    const int ri = threadIdx.x >> 4, c = threadIdx.x & 15;
    double* xcol = x + c0 + c;
    for (int i0 = 0; i0 < (int)rp; i0 += TI) {
        const int i = i0 + ri;
        if (i0 < c0 || i0 >= rank || c0 >= rank) {  // (the same decision in every thread of the workgroup)
            xcol[(int64_t)i * rp] = 0.0;
            continue;
        }
        const double* __restrict__ lrow = s + (int64_t)i * rp;
        double acc = (i == c0 + c) ? 1.0 : 0.0;
#pragma unroll 8
        for (int k = c0; k < i0; ++k) acc = fma(-lrow[k], xcol[(int64_t)k * rp], acc);
        lblk[ri][c] = (c <= ri) ? lrow[i0 + c] : 0.0;
        xb[ri][c] = acc;
        __syncthreads();
        if (ri == 0) {
            for (int r = 0; r < TI; ++r) {
                double t = xb[r][c];
                for (int q = 0; q < r; ++q) t = fma(-lblk[r][q], xb[q][c], t);
                xb[r][c] = t / lblk[r][r];
            }
        }
        __syncthreads();
        xcol[(int64_t)i * rp] = (i < rank && c0 + c < rank) ? xb[ri][c] : 0.0;
        __syncthreads();  // the rows just written feed the products of the next 16
    }
}

// out[i] = scale * sum_a (sum_{b <= a} X[a][b] F[b][i])^2 for the points i of this workgroup's slab of 64: the r x M product
// X F is never stored.  Per block of 128 rows of X, wave w owns rows 32 w .. 32 w + 31 (two MFMA row tiles) times the
// four 16-point tiles; the k loop stops at the wave's own diagonal (tiles above it are skipped), operands come straight
// from global / L2 as in k_gemm_nt_f64 (A = X, row-major with k contiguous: two 16-byte loads per lane and tile, the k
// index permuted the same way for both operands; B = F, point-contiguous: four 8-byte loads per tile, 128-byte runs per
// 16 lanes).  Each lane squares and adds its accumulators block after block, the four lane groups and the four waves are
// combined in a fixed order: no atomics, the same bytes on every run.
// MFMA maps as above: lane l supplies A[row l & 15][k l >> 4], B[k l >> 4][col l & 15]; C/D col = l & 15, row = (l >> 4) + 4 reg.
constexpr int SD_PTS = 64;
__global__ __launch_bounds__(kBlock) void k_lr_sigma_diag(const double* __restrict__ x, int64_t rp, int rank,
                                                          const double* __restrict__ f, int64_t ld, int64_t m,
                                                          double scale, double* __restrict__ out) {
    __shared__ double red[kBlock / 64][SD_PTS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, kq = lane >> 4;
    const int64_t p0 = (int64_t)blockIdx.x * SD_PTS;  // p0 + 63 < round_up(m, 256) = ld - 32: inside every row of F
    const int r16 = (rank + 15) & ~15;
    double ssum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int a0 = 0; a0 < rank; a0 += NB) {
        const int aw = a0 + 32 * wv;  // rows aw .. aw + 31 < rp (rp is a multiple of 128)
        if (aw >= rank) continue;     // (wave-uniform; no barrier inside the loop)
        d4 acc[2][4];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[t][j] = (d4){0.0, 0.0, 0.0, 0.0};
        const int kend = aw + 32 < r16 ? aw + 32 : r16;
        const double* __restrict__ xa = x + (int64_t)(aw + li) * rp + 4 * kq;
        for (int kc = 0; kc < kend; kc += 16) {
            d4 af[2];
            double bf[4][4];
            af[0] = *reinterpret_cast<const d4*>(xa + kc);
            af[1] = *reinterpret_cast<const d4*>(xa + 16 * rp + kc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = kc + 4 * kq + q;
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j][q] = k < rank ? f[(int64_t)k * ld + p0 + 16 * j + li] : 0.0;
            }
            const bool first = kc < aw + 16;  // the upper of the two row tiles ends one chunk earlier
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (first) acc[0][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[0][q], bf[j][q], acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[1][q], bf[j][q], acc[1][j], 0, 0, 0);
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) ssum[j] = fma(acc[t][j][r], acc[t][j][r], ssum[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double v = ssum[j];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (kq == 0) red[wv][16 * j + li] = v;
    }
    __syncthreads();
    if (threadIdx.x < SD_PTS) {
        const int64_t i = p0 + threadIdx.x;
        if (i < m) out[i] = scale * ((red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]));
    }
}

// resid, and nu where the caller gives one, into the staging block (*nu_dev: where, or nullptr); the pivot flag starts clear
int bcpd_stage_in(prg_cpd* h, const double* nu_hd, const double* resid_hd, int* info, double** nu_dev) {
    const int64_t m = h->M;
    hipStream_t st = h->stream;
    PRG_TRY(prg::ensure_stage(h, (size_t)m * 4 * sizeof(double)));
    *nu_dev = nullptr;
    PRG_HIP(hipMemcpyAsync(h->stage.p, resid_hd, (size_t)m * h->D * sizeof(double), hipMemcpyDefault, st));
    if (nu_hd) {
        *nu_dev = (double*)h->stage.p + (size_t)m * 3;
        PRG_HIP(hipMemcpyAsync(*nu_dev, nu_hd, (size_t)m * sizeof(double), hipMemcpyDefault, st));
    }
    PRG_HIP(hipMemsetAsync(info, 0, sizeof(int), st));
    return PRG_OK;
}

// v_hat (in W) and diag back in the caller's point order (diag by way of `tmp`, m doubles), then the pivot report
int bcpd_finish(prg_cpd* h, const double* diag, double* tmp, const int* info, double* vhat_hd, double* sigma_diag_hd) {
    const int64_t m = h->M;
    hipStream_t st = h->stream;
    double* stage = (double*)h->stage.p;
    k_unsort_rows<<<solve_grid1(m), kBlock, 0, st>>>(h->W.p, 3, h->D, m, h->perm_src.p, stage);
    PRG_HIP(hipMemcpyAsync(vhat_hd, stage, (size_t)m * h->D * sizeof(double), hipMemcpyDefault, st));
    k_unsort_rows<<<solve_grid1(m), kBlock, 0, st>>>(diag, 1, 1, m, h->perm_src.p, tmp);
    PRG_HIP(hipMemcpyAsync(sigma_diag_hd, tmp, (size_t)m * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipGetLastError());
    return prg::report_pivot(h, info, "prg_cpd_bcpd_solve");
}

// prg_cpd_bcpd_solve for a plan that holds the factor; the caller has checked the arguments and set the device
int bcpd_solve_lowrank(prg_cpd* h, double lmd, double cfac, const double* nu_hd, const double* resid_hd, double* vhat_hd,
                       double* sigma_diag_hd) {
    const int64_t m = h->M, ld = h->f_ld, mp = ld - 32;
    const int rank = h->f_rank;
    const prg::LowRankLayout L = prg::make_lowrank_layout(m, ld, rank);
    const prg::BcpdLowrankWs o = prg::bcpd_lowrank_ws(L);
    const int64_t rp = L.rp;
    PRG_TRY(prg::ensure_solve_workspace(h, o.total, true));
    double* const ws = h->nr_solve.p;
    double *S = ws + o.S, *X = ws + o.X, *part = ws + o.part, *upart = ws + o.upart, *b3 = ws + o.b3, *sp = ws + o.sp,
           *nu = ws + o.nu, *diag = ws + o.diag, *z = ws + o.z;
    int* info = reinterpret_cast<int*>(ws + o.info);
    const prg::SpdFactor fac{S, ws + o.linv, rp, rank, L.small};
    hipStream_t st = h->stream;

    double* nu_dev = nullptr;
    PRG_TRY(bcpd_stage_in(h, nu_hd, resid_hd, info, &nu_dev));
    k_bcpd_rhs<<<solve_grid1(ld), kBlock, 0, st>>>(h->rowacc.p, nu_dev, (const double*)h->stage.p, h->perm_src.p, m, ld, h->D, b3, sp, nu);
    // S = (lmd / c) I + F^T D F and z = F^T D R in one pass over the factor
    prg::k_lr_gram<<<dim3((unsigned)L.ntile, (unsigned)L.nsplit), kBlock, 0, st>>>(h->F.p, ld, m, rank, sp, nu, b3, L.chunk, part, upart);
    prg::k_lr_gram_reduce<<<solve_grid1(4 * std::max<int64_t>((int64_t)rp * rp, rp * 3)), kBlock, 0, st>>>(
        part, upart, L.ntile, L.nsplit, rank, rp, nullptr, lmd / cfac, S, z);
    PRG_TRY(prg::spd_factor(h->nr_queues, fac, info));
    PRG_TRY(prg::spd_solve3(h->nr_queues, fac, z));
    PRG_TRY(prg::lowrank_apply(h, z, h->W.p));  // v_hat = F S^-1 F^T D R, kept for the next transform
    k_tri_inverse<<<(unsigned)(rp / TI), kBlock, 0, st>>>(S, rp, rank, X);
    k_lr_sigma_diag<<<(unsigned)(mp / SD_PTS), kBlock, 0, st>>>(X, rp, rank, h->F.p, ld, m, 1.0 / cfac, diag);
    return bcpd_finish(h, diag, b3, info, vhat_hd, sigma_diag_hd);
}
}  // namespace

extern "C" int prg_cpd_bcpd_solve(prg_cpd* h, double lmd, double cfac, const double* nu_hd, const double* resid_hd,
                                  double* vhat_hd, double* sigma_diag_hd) {
    PRG_REQUIRE(h && h->bcpd && (h->G.p || h->F.p) && h->W.p, PRG_ERR_STATE, "prg_cpd_bcpd_solve: needs prg_cpd_bcpd_build_g first");
    PRG_REQUIRE(nu_hd || h->have_estep, PRG_ERR_STATE, "prg_cpd_bcpd_solve: no E-step has run and no nu was given");
    PRG_REQUIRE(resid_hd && vhat_hd && sigma_diag_hd, PRG_ERR_INVALID, "prg_cpd_bcpd_solve: NULL argument");
    PRG_REQUIRE(lmd > 0.0 && cfac > 0.0, PRG_ERR_INVALID, "prg_cpd_bcpd_solve: lmd and c must be > 0 (got %g, %g)", lmd,
                cfac);
    PRG_ENTER(h->device);
    if (h->F.p) return bcpd_solve_lowrank(h, lmd, cfac, nu_hd, resid_hd, vhat_hd, sigma_diag_hd);
    const int64_t m = h->M, mp = prg::round_up(m, NB), nblk = mp / NB;
    const prg::BcpdDenseWs o = prg::bcpd_dense_ws(m);
    PRG_TRY(prg::ensure_solve_workspace(h, o.total, false));
    double* const ws = h->nr_solve.p;
    double *S = ws + o.S, *wt = ws + o.wt, *b3 = ws + o.b3, *gb = ws + o.gb, *v = ws + o.v, *sp = ws + o.sp, *gt = ws + o.gt,
           *tv = ws + o.tv, *diag = ws + o.diag;
    int* info = reinterpret_cast<int*>(ws + o.info);
    const prg::SpdFactor fac{S, ws + o.linv, mp, m, false};
    hipStream_t st = h->stream;

    double* nu_dev = nullptr;
    PRG_TRY(bcpd_stage_in(h, nu_hd, resid_hd, info, &nu_dev));
    k_bcpd_rhs<<<solve_grid1(mp), kBlock, 0, st>>>(h->rowacc.p, nu_dev, (const double*)h->stage.p, h->perm_src.p, m, mp, h->D, b3,
                                                  sp);
    prg::k_build_s<<<dim3((unsigned)nblk, (unsigned)nblk), kBlock, 0, st>>>(h->G.p, m, mp, sp, nullptr, lmd / cfac, S);
    k_build_bt<<<dim3((unsigned)prg::ceil_div(mp, kBlock), (unsigned)std::min<int64_t>(mp, 32768)), kBlock, 0, st>>>(h->G.p, m, mp, sp, wt);
    PRG_TRY(prg::spd_factor(h->nr_queues, fac, info));
    PRG_TRY(prg::spd_right_solve(h->nr_queues, fac, wt, mp));  // Wt <- Wt L^-T
    k_sigma_diag<<<(unsigned)prg::ceil_div(m, 4), kBlock, 0, st>>>(wt, h->G.p, m, mp, lmd, diag);

    // v_hat = (c / lmd) (G b - G D^1/2 S^-1 D^1/2 G b)
    PRG_TRY(prg::nonrigid_gw(h, b3, gb));
    prg::k_scale_rows<<<solve_grid1(m), kBlock, 0, st>>>(sp, gb, m, v);
    if (mp > m) PRG_HIP(hipMemsetAsync(v + m * 3, 0, (size_t)(mp - m) * 3 * sizeof(double), st));
    PRG_TRY(prg::spd_solve3(h->nr_queues, fac, v));
    prg::k_scale_rows<<<solve_grid1(m), kBlock, 0, st>>>(sp, v, m, tv);
    PRG_TRY(prg::nonrigid_gw(h, tv, gt));
    k_bcpd_vhat<<<solve_grid1(m * 3), kBlock, 0, st>>>(gb, gt, m, cfac / lmd, h->W.p);
    return bcpd_finish(h, diag, gb, info, vhat_hd, sigma_diag_hd);
}
