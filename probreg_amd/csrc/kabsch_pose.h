// The Kabsch pose of a cross-covariance, shared by the refit of the global registration (global_reg.hip) and the
// point-to-point step of ICP (icp.hip).  Device only.  The text is shared, the bits are not: global_reg.hip compiles it under
// -ffp-contract=on, icp.hip under `#pragma clang fp contract(off)`, so the same cross-covariance gives poses that differ in the
// last bits between the two.  Both hold their poses to a bound, not to bytes.
#pragma once
#include "small_linalg.h"

namespace prg {

// Proper rotation (no scale) and shift from the cross-covariance hm[i][j] = sum (p - pm)_i (q - qm)_j: with hm = U S V^T the
// rotation is V diag(1, 1, det) U^T, the correction on the smallest singular value; pose = (R row-major, t = qm - R pm).
__device__ inline void kabsch_pose(const double hm[3][3], const double pm[3], const double qm[3], double pose[12]) {
    double U[3][3], V[3][3], sv[3];
    prg::jacobi_svd(hm, 3, U, V, sv);
    const double dd = prg::det3(U, 3) * prg::det3(V, 3) < 0.0 ? -1.0 : 1.0;
    double c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bool is_min = true;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j != k && (sv[j] < sv[k] || (sv[j] == sv[k] && j < k))) is_min = false;
        c[k] = is_min ? dd : 1.0;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double tr = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) r += c[k] * V[i][k] * U[j][k];
            pose[3 * i + j] = r;
            tr += r * pm[j];
        }
        pose[9 + i] = qm[i] - tr;
    }
}

}  // namespace prg
