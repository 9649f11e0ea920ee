// The closed-form M-steps of rigid and affine CPD as ONE device function: k_mstep (cpd.hip, one plan) and k_batch_mstep
// (cpd_batch.hip, one workgroup per problem of a batch) both run this body on one thread, so the two agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/probreg_hip.h"
#include "small_linalg.h"

namespace prg {
constexpr double kMstepEps32 = 1.1920928955078125e-07;  // np.finfo(np.float32).eps, cpd.py:189

// kind: PRG_TF_RIGID (cpd.py:160-192) or PRG_TF_AFFINE (cpd.py:219-244).  mom: MOMENTS, params: PARAMS (probreg_hip.h).
__device__ __forceinline__ void mstep_body(const double* __restrict__ mom, double* __restrict__ params, int kind,
                                           int update_scale, int dim) {
    // NB: every array index below is a compile-time constant after unrolling (run-time indices would push the
    // 3 x 3 arrays into scratch memory and cost ~1 us per access); the D = 2 case lives in the upper-left block
    // of the same 3 x 3 problem (z = 0 makes the third row / column of every moment vanish).
    const int d = dim;
    const double S0 = mom[0];
    double mu_x[3], mu_y[3], A[3][3], YPY[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        mu_x[i] = mom[1 + i] / S0;  // cpd.py:169
        mu_y[i] = mom[4 + i] / S0;  // cpd.py:170
    }
    // a = px^T (Y - mu_y) - mu_x (p1^T (Y - mu_y)) ; the second term is identically 0   (cpd.py:173-175)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i][j] = mom[7 + 3 * i + j] - mom[1 + i] * mu_y[j];
    const double syy[3][3] = {{mom[16], mom[17], mom[18]}, {mom[17], mom[19], mom[20]}, {mom[18], mom[20], mom[21]}};
    double tr_yp1y = 0.0, mux2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) YPY[i][j] = syy[i][j] - S0 * mu_y[i] * mu_y[j];  // (Y-mu)^T diag(p1) (Y-mu)
        tr_yp1y += YPY[i][i];
        mux2 += mu_x[i] * mu_x[i];
    }
    const double tr_xp1x = mom[22] - S0 * mux2;  // cpd.py:183 / 237
    double L[3][3], t[3];
    double scale = 1.0, sigma2, q;
    if (kind == PRG_TF_RIGID) {
        double U[3][3], V[3][3], sv[3];
        prg::jacobi_svd(A, d, U, V, sv);
        // rot = U diag(1,..,det(U V^T)) V^T with the correction on the smallest singular value (cpd.py:176-179)
        const double dd = prg::det3(U, d) * prg::det3(V, d);
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bool is_min = k < d;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < d && j != k && (sv[j] < sv[k] || (sv[j] == sv[k] && j < k))) is_min = false;
            c[k] = is_min ? dd : 1.0;
        }
        double tr_atr = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double r = 0;
#pragma unroll
                for (int k = 0; k < 3; ++k) r += c[k] * U[i][k] * V[j][k];
                L[i][j] = r;
                tr_atr += (i < d && j < d) ? A[i][j] * r : 0.0;  // trace(a^T rot), cpd.py:180
            }
        scale = update_scale ? tr_atr / tr_yp1y : 1.0;  // cpd.py:182
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double r = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) r += L[i][j] * mu_y[j];
            t[i] = (i < d) ? mu_x[i] - scale * r : 0.0;  // cpd.py:183
        }
        if (update_scale)
            sigma2 = (tr_xp1x - scale * tr_atr) / (S0 * d);  // cpd.py:186
        else
            sigma2 = (tr_xp1x + tr_yp1y - scale * tr_atr) / (S0 * d);  // cpd.py:188 (sic)
        sigma2 = fmax(sigma2, kMstepEps32);                                  // cpd.py:189
        q = (tr_xp1x - 2.0 * scale * tr_atr + scale * scale * tr_yp1y) / (2.0 * sigma2);
        q += d * S0 * 0.5 * log(sigma2);  // cpd.py:190-191
    } else {
        // b = solve(yp1y^T, a^T)^T : Gaussian elimination with partial pivoting (cpd.py:235) on the 3 x 3 embedding
        // [yp1y^T | a^T] with a unit diagonal in the unused dimension
        double Mx[3][6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const bool in = i < d && j < d;
                Mx[i][j] = in ? YPY[j][i] : ((i == j) ? 1.0 : 0.0);
                Mx[i][3 + j] = in ? A[j][i] : 0.0;
            }
        double ypy_scale = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) ypy_scale = fmax(ypy_scale, (i < d && j < d) ? fabs(YPY[i][j]) : 0.0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int r = c + 1; r < 3; ++r) {  // bring the largest pivot candidate up by conditional row swaps
                if (fabs(Mx[r][c]) > fabs(Mx[c][c])) {
#pragma unroll
                    for (int j = 0; j < 6; ++j) { const double tmp = Mx[c][j]; Mx[c][j] = Mx[r][j]; Mx[r][j] = tmp; }
                }
            }
            // np.linalg.solve raises on a singular matrix (cpd.py:237).  The moments are fp64 sums, so a rank-deficient
            // Y^T diag(p1) Y (fewer than D + 1 supported points, coplanar ones) shows up as a pivot at round-off
            // level of the matrix scale: turn it into the non-finite result the host maps to LinAlgError
            if (c < d && !(fabs(Mx[c][c]) > 1e-12 * ypy_scale)) Mx[c][c] = 0.0;
#pragma unroll
            for (int r = c + 1; r < 3; ++r) {
                const double f = Mx[r][c] / Mx[c][c];
#pragma unroll
                for (int j = 0; j < 6; ++j) Mx[r][j] -= (j >= c) ? f * Mx[c][j] : 0.0;
            }
        }
        double Xs[3][3];
#pragma unroll
        for (int col = 0; col < 3; ++col)
#pragma unroll
            for (int r = 2; r >= 0; --r) {
                double v = Mx[r][3 + col];
#pragma unroll
                for (int j = 0; j < 3; ++j) v -= (j > r) ? Mx[r][j] * Xs[j][col] : 0.0;
                Xs[r][col] = v / Mx[r][r];
            }
        double tr_ab = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double r = 0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const bool in = i < d && j < d;
                L[i][j] = in ? Xs[j][i] : ((i == j) ? 1.0 : 0.0);
                r += in ? L[i][j] * mu_y[j] : 0.0;
                tr_ab += in ? A[i][j] * L[i][j] : 0.0;  // trace(a b^T), cpd.py:238,240
            }
            t[i] = (i < d) ? mu_x[i] - r : 0.0;  // cpd.py:236
        }
        sigma2 = (tr_xp1x - tr_ab) / (S0 * d);  // cpd.py:239
        sigma2 = fmax(sigma2, kMstepEps32);
        q = (tr_xp1x - 2.0 * tr_ab + tr_ab) / (2.0 * sigma2) + d * S0 * 0.5 * log(sigma2);  // cpd.py:242-243
    }
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) params[3 * i + j] = L[i][j];
        params[9 + i] = t[i];
    }
    params[12] = scale;
    params[13] = sigma2;
    params[14] = q;
    params[15] = S0;
    params[16] += 1.0;
}
}  // namespace prg
