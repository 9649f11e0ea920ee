// The 3 x 3 symmetric eigenvector solve that the FPFH normals (csrc/fpfh.hip) and the plane refit (csrc/plane_seg.hip) share.
#pragma once
#include <hip/hip_runtime.h>

namespace prg {

// Eigenvector of the smallest eigenvalue of the symmetric matrix (xx, xy, xz, yy, yz, zz): cyclic Jacobi with
// compile-time indices only (small_linalg.h: a run-time index would move the arrays to scratch memory).
__device__ inline void smallest_eigenvector(const double c[6], double nrm[3]) {
    double a[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const double scale = fmax(fabs(a[0][0]), fmax(fabs(a[1][1]), fabs(a[2][2])));
    for (int sweep = 0; sweep < 30 && scale > 0.0; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (fabs(apq) <= 1.0e-20 * scale) {
                    a[p][q] = a[q][p] = 0.0;
                    continue;
                }
                rotated = true;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
                const int r = 3 - p - q;  // the third index (compile-time after unrolling)
                const double arp = a[r][p], arq = a[r][q];
                a[r][p] = a[p][r] = cs * arp - sn * arq;
                a[r][q] = a[q][r] = sn * arp + cs * arq;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = cs * vp - sn * vq;
                    V[i][q] = sn * vp + cs * vq;
                }
            }
        }
        if (!rotated) break;
    }
    int col = 0;  // smallest eigenvalue, ties to the lowest column
    if (a[1][1] < a[0][0]) col = 1;
    if (a[2][2] < (col == 1 ? a[1][1] : a[0][0])) col = 2;
    double v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = col == 0 ? V[i][0] : (col == 1 ? V[i][1] : V[i][2]);
    const double inv = 1.0 / sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double a0 = fabs(v[0]), a1 = fabs(v[1]), a2 = fabs(v[2]);
    const double lead = (a0 >= a1 && a0 >= a2) ? v[0] : (a1 >= a2 ? v[1] : v[2]);  // largest magnitude, ties: lowest axis
    const double sgn = lead < 0.0 ? -inv : inv;
#pragma unroll
    for (int i = 0; i < 3; ++i) nrm[i] = v[i] * sgn;
}

}  // namespace prg
