// Host build of the single-thread pose solves (tests/test_pose_host.py builds this with the host compiler under
// AddressSanitizer / UBSan and runs it; it is not linked against the HIP runtime): probreg_amd/csrc/small_linalg.h
// (jacobi_svd), kabsch_pose.h (the Kabsch pose of ICP and the global registration) and cpd_mstep.h (the rigid and affine
// M-steps of CPD), with __device__ defined away by the HIP headers' host branch.  The program computes, it does not judge:
// one record per line on stdin, one line of numbers at 17 digits per record on stdout.
//   SVD d a[9]                      ->  SVD    U[9] V[9] sv[3]
//   KABSCH hm[9] pm[3] qm[3]        ->  POSE   pose[12]
//   MSTEP kind update_scale dim mom[32]  ->  PARAMS params[17]      (kind: 0 rigid, 1 affine; params[16] starts at 0)
#include <stdio.h>
#include <string.h>

#include "../../probreg_amd/csrc/cpd_mstep.h"
#include "../../probreg_amd/csrc/kabsch_pose.h"
#include "../../probreg_amd/csrc/small_linalg.h"

static bool read_doubles(double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (scanf("%lf", &v[i]) != 1) return false;
    return true;
}

static void print_doubles(const char* tag, const double* v, int n) {
    printf("%s", tag);
    for (int i = 0; i < n; ++i) printf(" %.17g", v[i]);
    printf("\n");
}

int main() {
    char what[16];
    int records = 0;
    while (scanf("%15s", what) == 1) {
        if (strcmp(what, "SVD") == 0) {
            int d = 0;
            double a[3][3], out[21];
            if (scanf("%d", &d) != 1 || (d != 2 && d != 3) || !read_doubles(&a[0][0], 9)) return 2;
            double U[3][3], V[3][3], sv[3];
            prg::jacobi_svd(a, d, U, V, sv);
            memcpy(out, U, sizeof U);
            memcpy(out + 9, V, sizeof V);
            memcpy(out + 18, sv, sizeof sv);
            print_doubles("SVD", out, 21);
        } else if (strcmp(what, "KABSCH") == 0) {
            double hm[3][3], pm[3], qm[3], pose[12];
            if (!read_doubles(&hm[0][0], 9) || !read_doubles(pm, 3) || !read_doubles(qm, 3)) return 2;
            prg::kabsch_pose(hm, pm, qm, pose);
            print_doubles("POSE", pose, 12);
        } else if (strcmp(what, "MSTEP") == 0) {
            int kind = 0, update_scale = 0, dim = 0;
            double mom[PRG_NMOMENTS], params[PRG_NPARAMS];
            if (scanf("%d %d %d", &kind, &update_scale, &dim) != 3 || (dim != 2 && dim != 3) ||
                (kind != PRG_TF_RIGID && kind != PRG_TF_AFFINE) || !read_doubles(mom, PRG_NMOMENTS))
                return 2;
            for (int i = 0; i < PRG_NPARAMS; ++i) params[i] = 0.0;
            prg::mstep_body(mom, params, kind, update_scale, dim);
            print_doubles("PARAMS", params, 17);
        } else {
            fprintf(stderr, "pose_check: unknown record %s\n", what);
            return 2;
        }
        ++records;
    }
    printf("pose_check ok %d\n", records);
    return 0;
}
