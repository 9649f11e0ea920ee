// Tiny fp64 dense linear algebra used by the single-thread M-step kernels (device only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace prg {

// Columns G + 1 and G + 2 (cyclic) of m from its unit column G: the coordinate axis least aligned with that column,
// Gram-Schmidt, cross product.  m is then orthonormal with determinant +1.  Compile-time indices only (see jacobi_svd).
template <int G>
__device__ inline void complete_basis(double m[3][3]) {
    constexpr int p = (G + 1) % 3, q = (G + 2) % 3;
    const double a0 = fabs(m[0][G]), a1 = fabs(m[1][G]), a2 = fabs(m[2][G]);
    const int ax = (a0 <= a1 && a0 <= a2) ? 0 : ((a1 <= a2) ? 1 : 2);
    const double dp = (ax == 0) ? m[0][G] : ((ax == 1) ? m[1][G] : m[2][G]);
    double v[3], nn = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v[i] = ((i == ax) ? 1.0 : 0.0) - dp * m[i][G];
        nn += v[i] * v[i];
    }
    nn = 1.0 / sqrt(nn);
#pragma unroll
    for (int i = 0; i < 3; ++i) m[i][p] = v[i] * nn;
    m[0][q] = m[1][G] * m[2][p] - m[2][G] * m[1][p];
    m[1][q] = m[2][G] * m[0][p] - m[0][G] * m[2][p];
    m[2][q] = m[0][G] * m[1][p] - m[1][G] * m[0][p];
}

// One-sided Jacobi SVD of a d x d (d <= 3) matrix: a = U diag(sv) V^T.  Returns U, V, sv (unsorted).
// A column whose norm is at most 1e-14 of the largest one counts as zero: U is then completed to an orthonormal basis (one
// such column: cross product; two: Gram-Schmidt against the least aligned axis, for U and for V; all: the identity), so U
// and V are orthonormal for every rank.
// Supported range: the column norms are plain sums of squares, so the entries must keep their squares inside fp64 -
// roughly 1e-150 <= |a| <= 1e150 for the entries that matter.  Below that the squares underflow, alpha / beta / gamma
// become 0 and the result is silently the identity (a rank-0 answer); above it they overflow to inf and U is no longer
// orthonormal (|U U^T - I| of about 0.7 has been seen).  No point cloud gets near either end; tests/oracle_pose.py keeps
// its scaled families inside 2^-80 .. 2^80.
__device__ inline void jacobi_svd(const double a[3][3], int d, double U[3][3], double V[3][3], double sv[3]) {
    double g[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            g[i][j] = (i < d && j < d) ? a[i][j] : 0.0;
            V[i][j] = (i == j) ? 1.0 : 0.0;
        }
    // p, q loops are fully unrolled with compile-time indices so that g / V stay in registers
    // (run-time column indices would push the 3x3 arrays to scratch memory: 30 us instead of ~5)
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                if (q >= d) continue;
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    alpha += g[i][p] * g[i][p];
                    beta += g[i][q] * g[i][q];
                    gamma += g[i][p] * g[i][q];
                }
                const double ab = sqrt(alpha * beta);
                if (fabs(gamma) <= 1e-300 + 1e-17 * ab) continue;
                off = fmax(off, fabs(gamma) / ab);
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double gp = g[i][p], gq = g[i][q];
                    g[i][p] = c * gp - s * gq;
                    g[i][q] = s * gp + c * gq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        }
        if (off < 1e-15) break;
    }
    // Everything below uses compile-time array indices only (fully unrolled loops with predicates): a single
    // run-time index into g / U / V would move the 3 x 3 arrays to scratch memory (~1 us per access).
    double nmax = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double nn = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) nn += g[i][j] * g[i][j];
        sv[j] = (j < d) ? sqrt(nn) : 0.0;
        nmax = fmax(nmax, sv[j]);
    }
    bool ok[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        ok[j] = (j < d) && sv[j] > 1e-14 * nmax && sv[j] > 0.0;
        const double inv = ok[j] ? 1.0 / sv[j] : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) U[i][j] = ok[j] ? g[i][j] * inv : ((i == j) ? 1.0 : 0.0);
    }
    // complete U to an orthonormal basis where singular values vanish (rank-deficient `a`)
    if (d == 2) {
        if (ok[0] && !ok[1]) { U[0][1] = -U[1][0]; U[1][1] = U[0][0]; }
        else if (!ok[0] && ok[1]) { U[0][0] = U[1][1]; U[1][0] = -U[0][1]; }
        else if (!ok[0] && !ok[1]) { U[0][0] = U[1][1] = 1.0; U[0][1] = U[1][0] = 0.0; }
    } else if (d == 3) {
        const int nbad = (!ok[0]) + (!ok[1]) + (!ok[2]);
        if (nbad == 1) {
#pragma unroll
            for (int bcol = 0; bcol < 3; ++bcol) {
                if (ok[bcol]) continue;
                constexpr int nxt[3] = {1, 2, 0}, nx2[3] = {2, 0, 1};
                const int p = nxt[bcol], q = nx2[bcol];  // compile-time after unrolling
                U[0][bcol] = U[1][p] * U[2][q] - U[2][p] * U[1][q];
                U[1][bcol] = U[2][p] * U[0][q] - U[0][p] * U[2][q];
                U[2][bcol] = U[0][p] * U[1][q] - U[1][p] * U[0][q];
            }
        } else if (nbad == 3) {
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) U[i][j] = (i == j) ? 1.0 : 0.0;
        } else if (nbad == 2) {
            // V gets the same completion as U.  The sweeps leave its two null columns as some orthonormal basis of the null
            // space, turned by an angle that round-off decides (the two g columns they belong to are noise), and with them
            // the rotation U diag V^T about the one direction the data fix: two runs whose rank-1 matrices differ in the last
            // bit returned rotations half a turn apart.  With both completions taken from the good column alone the rotation
            // is a continuous function of the matrix (the sign of the good pair (u, v) cancels in every u_k v_k^T).
            if (ok[0]) { complete_basis<0>(U); complete_basis<0>(V); }
            else if (ok[1]) { complete_basis<1>(U); complete_basis<1>(V); }
            else { complete_basis<2>(U); complete_basis<2>(V); }
        }
    }
}

__device__ inline double det3(const double a[3][3], int d) {
    if (d == 2) return a[0][0] * a[1][1] - a[0][1] * a[1][0];
    return a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
           a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
}

}  // namespace prg
