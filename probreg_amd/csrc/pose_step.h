// The 6 x 6 Gauss-Newton step that ICP (csrc/icp.hip: point-to-plane, generalized) and fast global registration
// (csrc/fgr.hip) share: the Cholesky solve of the normal equations with its pivot rule, the pose of a twist, and the update
// of a pose by it.  Device code.  The including file switches contraction off (#pragma clang fp contract(off)) before it
// includes this header: every multiplication and addition here is rounded on its own.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace prg {

constexpr double kPivot = 1.0e-12;  // a Cholesky pivot <= kPivot max diag(A) is degenerate (part of the definition)

// x of A x = b by Cholesky, A from its upper triangle (row-major, 21), b = -g.  false: a pivot <= kPivot max diag(A).
__device__ inline bool cholesky6(const double* __restrict__ a21, const double* __restrict__ g, double (&x)[6]) {
    double L[6][6];
    int s = 0;
    double top = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            L[j][i] = a21[s++];
            if (i == j) top = fmax(top, L[i][i]);
        }
    const double floor_ = kPivot * top;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        double d = L[k][k];
#pragma unroll
        for (int j = 0; j < k; ++j) d -= L[k][j] * L[k][j];
        if (!(d > floor_)) return false;
        L[k][k] = sqrt(d);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            double v = L[i][k];
#pragma unroll
            for (int j = 0; j < k; ++j) v -= L[i][j] * L[k][j];
            L[i][k] = v / L[k][k];
        }
    }
    double w[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -g[i];
#pragma unroll
        for (int j = 0; j < i; ++j) v -= L[i][j] * w[j];
        w[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = w[i];
#pragma unroll
        for (int j = i + 1; j < 6; ++j) v -= L[j][i] * x[j];
        x[i] = v / L[i][i];
    }
    return true;
}

// Open3D's TransformVector6dToMatrix4d: d = (Rz(x2) Ry(x1) Rx(x0) row-major, shift (x3, x4, x5))
__device__ inline void twist_to_pose(const double (&x)[6], double (&d)[12]) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    d[0] = cg * cb; d[1] = cg * sb * sa - sg * ca; d[2] = cg * sb * ca + sg * sa;
    d[3] = sg * cb; d[4] = sg * sb * sa + cg * ca; d[5] = sg * sb * ca - cg * sa;
    d[6] = -sb;     d[7] = cb * sa;                d[8] = cb * ca;
    d[9] = x[3]; d[10] = x[4]; d[11] = x[5];
}

// pose <- d pose: R <- dR R, t <- dR t + dt (pose: 12 doubles, rotation row-major then shift)
__device__ inline void compose_pose(const double (&d)[12], double* __restrict__ pose) {
    double old[12];
    for (int k = 0; k < 12; ++k) old[k] = pose[k];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) pose[3 * a + b] = (d[3 * a] * old[b] + d[3 * a + 1] * old[3 + b]) + d[3 * a + 2] * old[6 + b];
        pose[9 + a] = ((d[3 * a] * old[9] + d[3 * a + 1] * old[10]) + d[3 * a + 2] * old[11]) + d[9 + a];
    }
}

}  // namespace prg
