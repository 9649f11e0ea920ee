// Blocked fp64 Cholesky factor / solve on MI355X (gfx950), interface in spd_solve.h: right-looking, NB = 128, trailing update
// and panel solve as NT-GEMMs on v_mfma_f64_16x16x4_f64.  fp64 throughout: cond(S) reaches 1e7-1e8 in the non-rigid and BCPD
// M-steps (cpd_nonrigid_solve.hip, cpd_bcpd_solve.hip), through which tests/test_dense_solve_gpu.py holds every schedule to LAPACK.
#include "spd_solve.h"

#include <math.h>

#include <algorithm>

#include "prg_common.h"

namespace {
constexpr int kBlock = 256;
constexpr int NB = prg::kSpdBlock;  // Cholesky block size == GEMM tile edge
constexpr int LDP = NB + 1;      // padded LDS row stride (doubles)
typedef double d4 __attribute__((ext_vector_type(4)));
using prg::SpdQueues;

// ---- diagonal block: Cholesky + triangular inverse in LDS ---------------------------------------
// One workgroup (256 threads), a = S[k0:k0+128, k0:k0+128] in 132 KB of LDS -> L (written back, lower) and
// L^-1 (to linv, full 128 x 128 row-major with an explicit zero upper triangle).
// Both phases are blocked by 8 columns so that the sequential part is 16 steps, not 128: the 8 x 8 diagonal
// block is factored / inverted redundantly by every thread in registers (36 doubles, static indexing), each
// thread then owns one row below it, and the rank-8 trailing update is register tiled 4 x 4.
constexpr int PB = 8;

// 1 / sqrt(d) for d > 0 to ~1 ulp: v_rsq_f64 (2^-26) + two Newton-Raphson steps, scaled against under/overflow of d y^2
__device__ __forceinline__ double rsqrt_newton(double d) {
    double y = __builtin_amdgcn_rsq(d);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = fma(-d * y, y, 1.0);  // 1 - d y^2
        y = fma(0.5 * y, e, y);
    }
    return y;
}

__device__ __forceinline__ void load_diag8(const double* a, int jb, double (&l)[PB][PB]) {
#pragma unroll
    for (int r = 0; r < PB; ++r)
#pragma unroll
        for (int c = 0; c < PB; ++c) l[r][c] = (c <= r) ? a[(jb + r) * LDP + jb + c] : 0.0;
}

// nreal: rows / columns of S that are not identity padding (>= k0 + 1): the block's trailing identity part is skipped.
__global__ __launch_bounds__(kBlock) void k_potrf_inv(double* __restrict__ s, int64_t ld, int64_t k0,
                                                      double* __restrict__ linv, int* __restrict__ info,
                                                      int64_t nreal) {
    // linv == nullptr: factor only (the small-system path solves with the factor itself, k_trsm_rows / k_tri_solve3)
    extern __shared__ double a[];  // [NB][LDP]
    __shared__ double rdiag[NB];   // 1 / L_jj
    const int tid = threadIdx.x;
    double* sblk = s + k0 * ld + k0;
    // active part of the block, in whole panels of 8 (the rest is identity and stays identity)
    const int nb = (int)((nreal - k0 >= NB) ? NB : ((nreal - k0 + PB - 1) / PB) * PB);
    // block -> LDS, 16 loads in flight per thread (a load / LDS-store pair per trip would pay one global round trip each)
    for (int base = 0; base < NB * NB; base += 16 * kBlock) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int idx = base + u * kBlock + tid, i = idx >> 7, j = idx & 127;
            v[u] = (i < nb && j < nb) ? sblk[(int64_t)i * ld + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int idx = base + u * kBlock + tid, i = idx >> 7, j = idx & 127;
            if (i < nb && j < nb) a[i * LDP + j] = v[u];
        }
    }
    // ---------------- Cholesky, 16 panels of 8 columns ----------------
    for (int jb = 0; jb < nb; jb += PB) {
        __syncthreads();
        double l[PB][PB];
        load_diag8(a, jb, l);
        const int i = jb + PB + tid;  // the row below the diagonal block this thread owns (if any)
        const bool has_row = i < nb;
        double x[PB];
        if (has_row) {
#pragma unroll
            for (int c = 0; c < PB; ++c) x[c] = a[i * LDP + jb + c];
        }
        __syncthreads();  // everybody holds the old diagonal block / its row in registers
        double inv[PB];
        bool bad = false;
#pragma unroll
        for (int c = 0; c < PB; ++c) {  // Cholesky-Crout on the 8 x 8 block
            double d = l[c][c];
#pragma unroll
            for (int k = 0; k < c; ++k) d -= l[c][k] * l[c][k];
            if (!(d > 0.0)) { bad = true; d = fabs(d) > 0.0 ? fabs(d) : 1.0; }
            // this chain is the sequential part of the whole factorisation: 1 / sqrt(d) from the hardware estimate and
            // two Newton steps (a dozen dependent operations) instead of a correctly rounded sqrt followed by a divide
            inv[c] = rsqrt_newton(d);
            l[c][c] = d * inv[c];
#pragma unroll
            for (int r = c + 1; r < PB; ++r) {
                double t = l[r][c];
#pragma unroll
                for (int k = 0; k < c; ++k) t -= l[r][k] * l[c][k];
                l[r][c] = t * inv[c];
            }
        }
        if (bad && tid == 0) atomicMax(info, (int)(k0 + jb + 1));
        if (has_row) {  // x := x * L11^-T  (forward substitution along the row)
#pragma unroll
            for (int c = 0; c < PB; ++c) {
                double t = x[c];
#pragma unroll
                for (int k = 0; k < c; ++k) t -= x[k] * l[c][k];
                x[c] = t * inv[c];
                a[i * LDP + jb + c] = x[c];
            }
        }
        if (tid == kBlock - 1) {
#pragma unroll
            for (int r = 0; r < PB; ++r) {
                rdiag[jb + r] = inv[r];
#pragma unroll
                for (int c = 0; c <= r; ++c) a[(jb + r) * LDP + jb + c] = l[r][c];
            }
        }
        __syncthreads();
        // rank-8 update of the trailing lower triangle, 4 x 4 register tiles
        const int t0 = jb + PB, nt = (nb - t0 + 3) >> 2;
        for (int t = tid; t < nt * nt; t += kBlock) {
            const int ti = t / nt, tk = t % nt;
            if (tk > ti) continue;
            const int i0 = t0 + 4 * ti, kk0 = t0 + 4 * tk;
            double ai[4][PB], ak[4][PB];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < PB; ++c) {
                    ai[r][c] = (i0 + r < nb) ? a[(i0 + r) * LDP + jb + c] : 0.0;
                    ak[r][c] = (kk0 + r < nb) ? a[(kk0 + r) * LDP + jb + c] : 0.0;
                }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (i0 + r < nb && kk0 + q <= i0 + r) {
                        double acc = 0.0;
#pragma unroll
                        for (int c = 0; c < PB; ++c) acc += ai[r][c] * ak[q][c];
                        a[(i0 + r) * LDP + kk0 + q] -= acc;
                    }
                }
        }
    }
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += kBlock) {
        const int i = idx >> 7, j = idx & 127;
        if (j <= i && i < nb) sblk[(int64_t)i * ld + j] = a[i * LDP + j];
    }
    if (!linv) return;
    // ---------------- in-place inverse of the lower triangle, block columns from last to first ----------------
    // with A11 the 8 x 8 diagonal block, A21 the rows below it and X22 = inv(A22) already in place:
    //   new A21 = -X22 * A21 * inv(A11),  new A11 = inv(A11)
    for (int jb = nb - PB; jb >= 0; jb -= PB) {
        __syncthreads();
        double l[PB][PB], li[PB][PB], dinv[PB];
        load_diag8(a, jb, l);
#pragma unroll
        for (int r = 0; r < PB; ++r) dinv[r] = rdiag[jb + r];
#pragma unroll
        for (int c = 0; c < PB; ++c) {  // li = inv(l), column by column (forward substitution)
#pragma unroll
            for (int r = 0; r < PB; ++r) {
                if (r < c) { li[r][c] = 0.0; continue; }
                double t = (r == c) ? 1.0 : 0.0;
#pragma unroll
                for (int k = 0; k < PB; ++k)
                    if (k >= c && k < r) t -= l[r][k] * li[k][c];
                li[r][c] = t * dinv[r];
            }
        }
        const int i = jb + PB + tid;
        const bool has_row = i < nb;
        double z[PB];
        if (has_row) {
            double y[PB];
#pragma unroll
            for (int c = 0; c < PB; ++c) y[c] = 0.0;
            // y = X22[i, :] * A21 (X22 lower triangular); four rows per trip so that their LDS reads are in flight together
            int k = jb + PB;
            for (; k + 3 <= i; k += 4) {
                double xk[4], ar[4][PB];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xk[u] = a[i * LDP + k + u];
#pragma unroll
                    for (int c = 0; c < PB; ++c) ar[u][c] = a[(k + u) * LDP + jb + c];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int c = 0; c < PB; ++c) y[c] = fma(xk[u], ar[u][c], y[c]);
            }
            for (; k <= i; ++k) {
                const double xik = a[i * LDP + k];
#pragma unroll
                for (int c = 0; c < PB; ++c) y[c] = fma(xik, a[k * LDP + jb + c], y[c]);
            }
#pragma unroll
            for (int c = 0; c < PB; ++c) {  // z = -y * inv(A11)
                double t = 0.0;
#pragma unroll
                for (int q = 0; q < PB; ++q)
                    if (q >= c) t += y[q] * li[q][c];
                z[c] = -t;
            }
        }
        __syncthreads();  // every read of the old A21 / A11 is done
        if (has_row) {
#pragma unroll
            for (int c = 0; c < PB; ++c) a[i * LDP + jb + c] = z[c];
        }
        if (tid == kBlock - 1) {
#pragma unroll
            for (int r = 0; r < PB; ++r)
#pragma unroll
                for (int c = 0; c <= r; ++c) a[(jb + r) * LDP + jb + c] = li[r][c];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += kBlock) {
        const int i = idx >> 7, j = idx & 127;
        linv[idx] = (i < nb) ? ((j <= i) ? a[i * LDP + j] : 0.0) : (i == j ? 1.0 : 0.0);
    }
}

// ---- NT GEMM on the f64 matrix cores ---------------------------------------------------------------
// C[i][j] (op)= sum_{k < K} A[i][k] * B[j][k] for one 128 x 128 tile per workgroup, K a multiple of 16.
//   MODE 0 (panel solve, X = A21 * Linv^T, K = 128): C = A B^T, C aliases A (all loads finish before any store).
//   MODE 1 (trailing update, A22 -= L21 L21^T): C -= A B^T on the lower tiles, 1-D triangular grid.
//   MODE 2 (update inside the outer panel): C -= A B^T on a (rows x few column tiles) grid, tiles above the
//           diagonal skipped.
// The outer panel is 512 columns wide (4 Cholesky blocks): the big MODE 1 update then runs with K = 512, i.e.
// 4x fewer read-modify-write passes over the trailing matrix than with K = 128 - at K = 128 the update is
// HBM bound (16 flop per byte of C traffic), at K = 512 it is bound by the matrix cores.
// Wave w owns the 64 x 64 quadrant (w>>1, w&1) as 4 x 4 MFMA tiles of 16 x 16 (64 accumulator f64
// per lane).  v_mfma_f64_16x16x4_f64 operand map: lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15]; the k index inside a 16-chunk is permuted (lane group kq holds
// k = 4 kq + s at step s) identically for A and B, so every lane fetches 4 consecutive doubles
// (two 16-byte loads) per 16-row strip.  C/D map: col = l&15, row = (l>>4) + 4 reg.
template <int MODE>
__global__ __launch_bounds__(kBlock, 2) void k_gemm_nt_f64(const double* abase, const double* bbase,
                                                        int64_t lda, int64_t ldb, double* cbase, int64_t ldc,
                                                        int kdim) {
    int by, bx;
    if (MODE == 2 || MODE == 3) {  // MODE 3: rectangular C -= A B^T, every tile (triangular solve with many RHS)
        by = blockIdx.x;
        bx = blockIdx.y;
        if (MODE == 2 && bx > by) return;
    } else if (MODE == 1) {
        const int t = blockIdx.x;
        by = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
        while ((int64_t)(by + 1) * (by + 2) / 2 <= t) ++by;
        while ((int64_t)by * (by + 1) / 2 > t) --by;
        bx = t - (int)((int64_t)by * (by + 1) / 2);
    } else {
        by = blockIdx.x;
        bx = 0;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = wv >> 1, wc = wv & 1;
    const int li = lane & 15, kq = lane >> 4;
    const double* ap = abase + ((int64_t)by * NB + wr * 64 + li) * lda + 4 * kq;
    const double* bp = bbase + ((int64_t)bx * NB + wc * 64 + li) * ldb + 4 * kq;
    d4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < kdim; kc += 16) {
        // operands straight from global / L2 into registers; with two workgroups per CU the loads of one wave
        // overlap the 64 MFMAs (64 cycles each) of the other wave on the same SIMD
        d4 af[4], bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            af[t] = *reinterpret_cast<const d4*>(ap + (int64_t)t * 16 * lda + kc);
            bf[t] = *reinterpret_cast<const d4*>(bp + (int64_t)t * 16 * ldb + kc);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i][s], bf[j][s], acc[i][j], 0, 0, 0);
    }
    if (MODE == 0) __syncthreads();  // C aliases A: every wave's loads are done before anyone stores
    // epilogue: the read-modify-write of the C tile is batched (16 independent loads in flight, then 16
    // stores) - a load/sub/store chain per element would serialise 64 global round trips per lane
    double* __restrict__ cp = cbase + ((int64_t)by * NB + wr * 64 + kq) * ldc + (int64_t)bx * NB + wc * 64 + li;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (MODE != 0) {
            double cv[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) cv[j][r] = cp[(int64_t)(16 * i + 4 * r) * ldc + 16 * j];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) cp[(int64_t)(16 * i + 4 * r) * ldc + 16 * j] = cv[j][r] - acc[i][j][r];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) cp[(int64_t)(16 * i + 4 * r) * ldc + 16 * j] = acc[i][j][r];
        }
    }
}

// ---- small systems: solves with the factor itself (no block inverses) ------------------------------------------------
// The reduced system of the low-rank M-step has a few hundred rows: the triangular inverse that feeds the MFMA panel
// solve of the big factorisation costs more than it saves there (it is 60 % of k_potrf_inv).
//
// Panel solve X L11^T = A21 for the rows below a factored diagonal block, in place.  8 lanes share a row (lane s owns the
// columns j = s mod 8); right-looking: x_j is finished by its owner, broadcast inside the 8-lane group, and every lane
// retires it from its later columns.  L11 sits in LDS (k * LDP + j: conflict free across the 8 x 8 lanes of a wave).
__global__ __launch_bounds__(kBlock) void k_trsm_rows(double* __restrict__ s, int64_t ld, int64_t k0, int64_t row_begin,
                                                      int64_t row_end) {
    extern __shared__ double a[];  // [NB][LDP] lower triangle of L11
    __shared__ double rdiag[NB];
    const int tid = threadIdx.x;
    const double* lblk = s + k0 * ld + k0;
    for (int base = 0; base < NB * NB; base += 16 * kBlock) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int idx = base + u * kBlock + tid, i = idx >> 7, j = idx & 127;
            v[u] = j <= i ? lblk[(int64_t)i * ld + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int idx = base + u * kBlock + tid, i = idx >> 7, j = idx & 127;
            a[i * LDP + j] = v[u];
        }
    }
    __syncthreads();
    if (tid < NB) rdiag[tid] = 1.0 / a[tid * LDP + tid];
    __syncthreads();
    const int sub = tid & 7;
    const int64_t row = row_begin + (int64_t)blockIdx.x * (kBlock / 8) + (tid >> 3);
    const bool live = row < row_end;
    double* __restrict__ arow = s + (live ? row : row_begin) * ld + k0;
    double x[16];  // columns sub + 8 q
#pragma unroll
    for (int q = 0; q < 16; ++q) x[q] = live ? arow[sub + 8 * q] : 0.0;
    const int lane = tid & 63;
#pragma unroll
    for (int jq = 0; jq < 16; ++jq) {
#pragma unroll
        for (int js = 0; js < 8; ++js) {
            const int j = 8 * jq + js;
            const double mine = x[jq] * rdiag[j];  // only lane js of the group holds column j
            const double xj = __shfl(mine, (lane & ~7) | js, 64);
            if (sub == js) x[jq] = xj;
#pragma unroll
            for (int q = jq; q < 16; ++q) {
                const int k = sub + 8 * q;
                if (k > j) x[q] = fma(-xj, a[k * LDP + j], x[q]);
            }
        }
    }
    if (live) {
#pragma unroll
        for (int q = 0; q < 16; ++q) arow[sub + 8 * q] = x[q];
    }
}

// L11 u = v (TRANS 0) or L11^T u = v (TRANS 1) for one diagonal block and 3 right-hand sides, in place: one wave, two rows
// per lane, column oriented - u_j is finished by its owner, broadcast, and retired from the rows that still wait.
template <int TRANS>
__global__ __launch_bounds__(kBlock) void k_tri_solve3(const double* __restrict__ s, int64_t ld, int64_t k0,
                                                       double* __restrict__ v) {
    extern __shared__ double a[];  // [NB][LDP]
    const int tid = threadIdx.x;
    const double* lblk = s + k0 * ld + k0;
    for (int base = 0; base < NB * NB; base += 16 * kBlock) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int idx = base + u * kBlock + tid, i = idx >> 7, j = idx & 127;
            t[u] = j <= i ? lblk[(int64_t)i * ld + j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int idx = base + u * kBlock + tid, i = idx >> 7, j = idx & 127;
            a[i * LDP + j] = t[u];
        }
    }
    __syncthreads();
    if (tid >= 64) return;
    const int lane = tid;
    double r[2][3], dinv[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        dinv[h] = 1.0 / a[k * LDP + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[h][c] = v[(k0 + k) * 3 + c];
    }
#pragma unroll
    for (int h0 = 0; h0 < 2; ++h0) {
        const int hj = TRANS ? 1 - h0 : h0;  // the half the pivots of this sweep live in
        for (int step = 0; step < 64; ++step) {
            const int jl = TRANS ? 63 - step : step, j = jl + 64 * hj;
            double u[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] = __shfl(r[hj][c] * dinv[hj], jl, 64);
            if (lane == jl) {
#pragma unroll
                for (int c = 0; c < 3; ++c) r[hj][c] = u[c];
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int k = lane + 64 * h;
                const bool pending = TRANS ? k < j : k > j;
                const double l = pending ? (TRANS ? a[j * LDP + k] : a[k * LDP + j]) : 0.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) r[h][c] = fma(-l, u[c], r[h][c]);
            }
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[(k0 + lane + 64 * h) * 3 + c] = r[h][c];
}

// ---- block triangular solves with 3 right-hand sides ----------------------------------------------
// L_k x = v_k (TRANS = 0) or L_k^T x = v_k (TRANS = 1) for the diagonal block at k0; v, x are [mp][3] row-major.
// x0 = Linv_k v_k alone is only conditionally stable: its residual grows with cond(L_k) (~1e3 late in a registration),
// where substitution's does not, and G W came out a digit further from LAPACK than W itself.  One step of refinement
// against the factor, x = x0 + Linv_k (v_k - L_k x0), brings the block solve to substitution level at the price of two
// more 128 x 128 products in a kernel that is bound by its launch.
template <int TRANS>
__global__ __launch_bounds__(384) void k_diag_solve(const double* __restrict__ linv, const double* __restrict__ s,
                                                    int64_t ld, double* __restrict__ v, int64_t k0) {
    __shared__ double vin[NB][3], x0[NB][3];
    const int r = threadIdx.x / 3, c = threadIdx.x % 3;
    const double* __restrict__ lblk = s + k0 * ld + k0;  // L_k in the lower triangle (above it: what S held before)
    const double vr = v[(k0 + r) * 3 + c];
    vin[r][c] = vr;
    __syncthreads();
    // the upper triangle of linv is stored as explicit zeros, so the loops can run over all 128 terms
    // with independent loads (unrolled, pipelined) instead of a data-dependent trip count
    auto apply_inverse = [&]() {
        double acc = 0.0;
        if (TRANS == 0) {
#pragma unroll 16
            for (int k = 0; k < NB; ++k) acc += linv[r * NB + k] * vin[k][c];
        } else {
#pragma unroll 16
            for (int k = 0; k < NB; ++k) acc += linv[k * NB + r] * vin[k][c];
        }
        return acc;
    };
    const double xr = apply_inverse();
    x0[r][c] = xr;
    __syncthreads();
    double res = vr;
    if (TRANS == 0) {
#pragma unroll 16
        for (int k = 0; k < NB; ++k) res = fma(-(k <= r ? lblk[(int64_t)r * ld + k] : 0.0), x0[k][c], res);
    } else {
#pragma unroll 16
        for (int k = 0; k < NB; ++k) res = fma(-(k >= r ? lblk[(int64_t)k * ld + r] : 0.0), x0[k][c], res);
    }
    vin[r][c] = res;  // (every thread read its own entry of vin only since the barrier)
    __syncthreads();
    v[(k0 + r) * 3 + c] = xr + apply_inverse();
}

// forward (right-looking): v[i] -= sum_c L[i][k0 + c] * x_k[c] for rows i >= k0 + 128.
// 4 threads per row, each covering 32 of the 128 columns in 16-byte pieces; x_k in LDS.
__global__ __launch_bounds__(kBlock) void k_fwd_update(const double* __restrict__ s, int64_t ld, int64_t k0,
                                                       int64_t mp, double* __restrict__ v) {
    __shared__ double xk[NB][3];
    for (int idx = threadIdx.x; idx < NB * 3; idx += kBlock) xk[idx / 3][idx % 3] = v[k0 * 3 + idx];
    __syncthreads();
    const int part = threadIdx.x & 3;
    const int64_t i = k0 + NB + (int64_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (i < mp) {
        const double* row = s + i * ld + k0;
#pragma unroll 4
        for (int q = 0; q < 16; ++q) {
            const int c = q * 8 + part * 2;
            const double2 l2 = *reinterpret_cast<const double2*>(row + c);
            a0 += l2.x * xk[c][0] + l2.y * xk[c + 1][0];
            a1 += l2.x * xk[c][1] + l2.y * xk[c + 1][1];
            a2 += l2.x * xk[c][2] + l2.y * xk[c + 1][2];
        }
    }
    a0 += __shfl_xor(a0, 1, 64); a0 += __shfl_xor(a0, 2, 64);
    a1 += __shfl_xor(a1, 1, 64); a1 += __shfl_xor(a1, 2, 64);
    a2 += __shfl_xor(a2, 1, 64); a2 += __shfl_xor(a2, 2, 64);
    if (i < mp && part == 0) {
        v[i * 3] -= a0;
        v[i * 3 + 1] -= a1;
        v[i * 3 + 2] -= a2;
    }
}

// backward (right-looking): v[c] -= sum_r L[k0 + r][c] * x_k[r] for columns c < k0 (coalesced along c).
__global__ __launch_bounds__(kBlock) void k_bwd_update(const double* __restrict__ s, int64_t ld, int64_t k0,
                                                       double* __restrict__ v) {
    __shared__ double xk[NB][3];
    for (int idx = threadIdx.x; idx < NB * 3; idx += kBlock) xk[idx / 3][idx % 3] = v[k0 * 3 + idx];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= k0) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    const double* col = s + k0 * ld + c;
#pragma unroll 8
    for (int r = 0; r < NB; ++r) {
        const double l = col[(int64_t)r * ld];
        a0 += l * xk[r][0];
        a1 += l * xk[r][1];
        a2 += l * xk[r][2];
    }
    v[c * 3] -= a0;
    v[c * 3 + 1] -= a1;
    v[c * 3 + 2] -= a2;
}
inline dim3 grid1(int64_t n) { return dim3((unsigned)prg::ceil_div(n, kBlock)); }

// blocked Cholesky S = L L^T (lower, in place): outer panels of 512 columns, inner blocks of 128; the inverses
// of the diagonal blocks go to linv.  Enqueued on the main stream (+ the side stream of the look-ahead); on
// return the main stream waits for everything.
int cholesky_lookahead(SpdQueues& q, double* S, int64_t mp, double* linv, int* info, int64_t nreal) {
    hipStream_t st = q.main;
    // Look-ahead over two streams: the trailing update of outer panel J is split into U1 (the 512 columns of
    // the next panel, main stream) and U2 (everything to the right, side stream), so the latency-bound panel
    // factorisation J+1 (potrf + panel solves) runs underneath U2(J) instead of leaving the GPU idle.
    const size_t lds = (size_t)NB * LDP * sizeof(double);
    constexpr int64_t NBO = 512;
    const int64_t nouter = prg::ceil_div(mp, NBO);
    if (!q.side) PRG_HIP(hipStreamCreateWithFlags(&q.side, hipStreamNonBlocking));
    while ((int64_t)q.events.size() < 2 * nouter + 1) {
        hipEvent_t e;
        PRG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        q.events.push_back(e);
    }
    hipStream_t sb = q.side;
    PRG_HIP(hipEventRecord(q.events[2 * nouter], st));
    PRG_HIP(hipStreamWaitEvent(sb, q.events[2 * nouter], 0));
    int64_t last_u2 = -1;
    for (int64_t J = 0; J < nouter; ++J) {
        const int64_t K0 = J * NBO;
        const int64_t kend = std::min<int64_t>(K0 + NBO, mp);
        for (int64_t k0 = K0; k0 < kend; k0 += NB) {
            double* lk = linv + (size_t)(k0 / NB) * NB * NB;
            k_potrf_inv<<<1, kBlock, lds, st>>>(S, mp, k0, lk, info, nreal);
            const int64_t below = (mp - k0 - NB) / NB;
            if (below > 0) {
                double* a21 = S + (k0 + NB) * mp + k0;
                k_gemm_nt_f64<0><<<(unsigned)below, kBlock, 0, st>>>(a21, lk, mp, NB, a21, mp, NB);
                const int64_t inner_cols = (kend - k0 - NB) / NB;  // remaining block columns of the outer panel
                if (inner_cols > 0)
                    k_gemm_nt_f64<2><<<dim3((unsigned)below, (unsigned)inner_cols), kBlock, 0, st>>>(
                        a21, a21, mp, mp, S + (k0 + NB) * mp + (k0 + NB), mp, NB);
            }
        }
        const int64_t rem = (mp - kend) / NB;
        if (rem <= 0) break;
        const int kd = (int)(kend - K0);
        double* apan = S + kend * mp + K0;  // rows >= kend of the outer panel: L[kend:, K0:kend]
        PRG_HIP(hipEventRecord(q.events[2 * J], st));
        // U2(J): the sub-triangle right of the next panel, on the side stream
        const int64_t r2 = rem - NBO / NB;
        if (r2 > 0) {
            PRG_HIP(hipStreamWaitEvent(sb, q.events[2 * J], 0));
            double* ap2 = apan + (NBO / NB) * NB * mp;
            k_gemm_nt_f64<1><<<(unsigned)(r2 * (r2 + 1) / 2), kBlock, 0, sb>>>(
                ap2, ap2, mp, mp, S + (kend + NBO) * mp + (kend + NBO), mp, kd);
            PRG_HIP(hipEventRecord(q.events[2 * J + 1], sb));
        }
        // U1(J): the next panel's columns; it must see U2(J-1), which updated the same tiles
        if (last_u2 >= 0) PRG_HIP(hipStreamWaitEvent(st, q.events[2 * last_u2 + 1], 0));
        k_gemm_nt_f64<2><<<dim3((unsigned)rem, (unsigned)std::min<int64_t>(NBO / NB, rem)), kBlock, 0, st>>>(
            apan, apan, mp, mp, S + kend * mp + kend, mp, kd);
        last_u2 = (r2 > 0) ? J : -1;
    }
    if (last_u2 >= 0) PRG_HIP(hipStreamWaitEvent(st, q.events[2 * last_u2 + 1], 0));
    return PRG_OK;
}

// Small SPD systems (the r x r system of the low-rank M-step): plain right-looking blocked Cholesky on one stream, the
// factor is used as it is.  nreal: rows that are not identity padding.
int cholesky_small(SpdQueues& q, double* S, int64_t mp, int* info, int64_t nreal) {
    hipStream_t st = q.main;
    const size_t lds = (size_t)NB * LDP * sizeof(double);
    for (int64_t k0 = 0; k0 < mp && k0 < nreal; k0 += NB) {
        k_potrf_inv<<<1, kBlock, lds, st>>>(S, mp, k0, nullptr, info, nreal);
        const int64_t row_end = std::min<int64_t>(mp, prg::round_up(nreal, NB));  // identity rows need nothing
        const int64_t rows = row_end - (k0 + NB);
        if (rows <= 0) break;
        k_trsm_rows<<<(unsigned)prg::ceil_div(rows, kBlock / 8), kBlock, lds, st>>>(S, mp, k0, k0 + NB, row_end);
        const int64_t below = rows / NB;
        double* a21 = S + (k0 + NB) * mp + k0;
        k_gemm_nt_f64<2><<<dim3((unsigned)below, (unsigned)below), kBlock, 0, st>>>(a21, a21, mp, mp,
                                                                                  S + (k0 + NB) * mp + (k0 + NB), mp, NB);
    }
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

}  // namespace

namespace prg {

int spd_prepare() {
    for (const void* fn : {reinterpret_cast<const void*>(k_potrf_inv), reinterpret_cast<const void*>(k_trsm_rows),
                           reinterpret_cast<const void*>(k_tri_solve3<0>), reinterpret_cast<const void*>(k_tri_solve3<1>)})
        PRG_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, NB * LDP * (int)sizeof(double)));
    return PRG_OK;
}

int spd_factor(SpdQueues& q, const SpdFactor& f, int* info) {
    return f.small ? cholesky_small(q, f.S, f.ld, info, f.nreal) : cholesky_lookahead(q, f.S, f.ld, f.linv, info, f.nreal);
}

// Block forward and backward sweep.  A diagonal block is solved with its inverse and one refinement step (k_diag_solve) or,
// for a small factor, by substitution (k_tri_solve3); a small factor's identity blocks beyond nreal are skipped (u = v).
int spd_solve3(SpdQueues& q, const SpdFactor& f, double* v) {
    hipStream_t st = q.main;
    const size_t lds = (size_t)NB * LDP * sizeof(double);
    const int64_t mp = f.ld, nblk = f.small ? ceil_div(std::min(mp, f.nreal), NB) : mp / NB, end = nblk * NB;
    for (int64_t kb = 0; kb < nblk; ++kb) {  // L u' = v
        const int64_t k0 = kb * NB, rows = end - k0 - NB;
        if (f.small)
            k_tri_solve3<0><<<1, kBlock, lds, st>>>(f.S, mp, k0, v);
        else
            k_diag_solve<0><<<1, 384, 0, st>>>(f.linv + (size_t)kb * NB * NB, f.S, mp, v, k0);
        if (rows > 0) k_fwd_update<<<(unsigned)ceil_div(rows, 64), kBlock, 0, st>>>(f.S, mp, k0, end, v);
    }
    for (int64_t kb = nblk - 1; kb >= 0; --kb) {  // L^T u = u'
        const int64_t k0 = kb * NB;
        if (f.small)
            k_tri_solve3<1><<<1, kBlock, lds, st>>>(f.S, mp, k0, v);
        else
            k_diag_solve<1><<<1, 384, 0, st>>>(f.linv + (size_t)kb * NB * NB, f.S, mp, v, k0);
        if (k0 > 0) k_bwd_update<<<grid1(k0), kBlock, 0, st>>>(f.S, mp, k0, v);
    }
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

// Left-looking over panels of k 128-column blocks: one K-deep rectangular update with everything to the left of the
// panel, then k (update inside the panel, multiply by the inverted diagonal block) steps.
// The update runs nblk x k workgroups, 512 at a time (two per CU): k is chosen so that this is close to a whole
// number of rounds - at 20k rows (157 block rows) four blocks per panel would leave the second round 23 % full.
int spd_right_solve(SpdQueues& q, const SpdFactor& f, double* wt, int64_t rows) {
    hipStream_t st = q.main;
    const int64_t mp = f.ld, nblk = rows / NB;
    int kpanel = 4;
    {
        double best = 1e30;
        for (int k = 4; k <= 16; ++k) {
            const double wgs = (double)nblk * k;
            const double waste = ceil(wgs / 512.0) * 512.0 / wgs;
            if (waste <= best + 1e-9) {  // ties: the wider panel (fewer, larger launches)
                best = waste;
                kpanel = k;
            }
        }
    }
    const int64_t NBO = (int64_t)kpanel * NB;
    for (int64_t K0 = 0; K0 < mp; K0 += NBO) {
        const int64_t kend = std::min<int64_t>(K0 + NBO, mp);
        if (K0 > 0)
            k_gemm_nt_f64<3><<<dim3((unsigned)nblk, (unsigned)((kend - K0) / NB)), kBlock, 0, st>>>(
                wt, f.S + K0 * mp, mp, mp, wt + K0, mp, (int)K0);
        for (int64_t k0 = K0; k0 < kend; k0 += NB) {
            if (k0 > K0)
                k_gemm_nt_f64<3><<<dim3((unsigned)nblk, 1u), kBlock, 0, st>>>(wt + K0, f.S + k0 * mp + K0, mp, mp, wt + k0, mp,
                                                                             (int)(k0 - K0));
            k_gemm_nt_f64<0><<<(unsigned)nblk, kBlock, 0, st>>>(wt + k0, f.linv + (size_t)(k0 / NB) * NB * NB, mp, NB,
                                                               wt + k0, mp, NB);
        }
    }
    return PRG_OK;
}

void spd_release(SpdQueues& q) {
    for (hipEvent_t e : q.events) (void)hipEventDestroy(e);
    q.events.clear();
    if (q.side) (void)hipStreamDestroy(q.side);
    q.side = nullptr;
}

}  // namespace prg
