// Blocked fp64 Cholesky factor / solve of a padded SPD matrix on the f64 matrix cores (spd_solve.hip).  Knows nothing of CPD:
// the caller owns the matrix, the block inverses, the pivot flag and the queues.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace prg {
constexpr int kSpdBlock = 128;  // Cholesky block == GEMM tile edge; ld and every row count are multiples of it

// `side` and `events` are the look-ahead factorisation's, created on first use; the owner keeps them until spd_release.
struct SpdQueues {
    hipStream_t main = nullptr, side = nullptr;
    std::vector<hipEvent_t> events;
};
// S [ld][ld] row-major, lower triangle, identity beyond the `nreal` real rows; factored in place.
//   small: right-looking on the main stream, the solves substitute with the factor itself; linv is not touched
//   else:  look-ahead over both streams; linv [ld / 128][128][128] receives the inverted diagonal blocks
struct SpdFactor {
    double *S, *linv;
    int64_t ld, nreal;
    bool small;
};
int spd_prepare();  // the opt-in above 64 KB of LDS for the kernels that hold a 128 x 129 block: before their first launch
int spd_factor(SpdQueues& q, const SpdFactor& f, int* info);  // first non-positive pivot + 1 is max-ed into *info (device)
int spd_solve3(SpdQueues& q, const SpdFactor& f, double* v);  // L L^T u = v in place, v [ld][3] row-major
int spd_right_solve(SpdQueues& q, const SpdFactor& f, double* wt, int64_t rows);  // Wt <- Wt L^-T, wt [rows][ld]; not small
void spd_release(SpdQueues& q);
}  // namespace prg
