// What the two solve drivers of the CPD plan share (cpd_nonrigid_solve.hip: non-rigid M-step, cpd_bcpd_solve.hip: BCPD solve);
// everything here is defined in cpd_nonrigid_solve.hip.
#pragma once
#include "cpd_plan.h"
#include "cpd_solve_layout.h"

namespace prg {
static_assert(kSolveNB == kSpdBlock, "the workspace is laid out in the solver's blocks");
inline dim3 solve_grid1(int64_t n) { return dim3((unsigned)ceil_div(n, kSolveThreads)); }

__global__ void k_build_s(const float* __restrict__ g, int64_t m, int64_t mp, const double* __restrict__ sp,
                          const double* __restrict__ params, double lmd, double* __restrict__ s);
__global__ void k_scale_rows(const double* __restrict__ sp, const double* __restrict__ in, int64_t mp, double* __restrict__ out);
__global__ void k_lr_gram(const double* __restrict__ f, int64_t ld, int64_t m, int rank, const double* __restrict__ sp,
                          const double* __restrict__ dw, const double* __restrict__ b3, int64_t chunk, double* __restrict__ part,
                          double* __restrict__ upart);
__global__ void k_lr_gram_reduce(const double* __restrict__ part, const double* __restrict__ upart, int ntile, int nsplit,
                                 int rank, int64_t rp, const double* __restrict__ params, double lmd, double* __restrict__ s,
                                 double* __restrict__ u);

// The workspace of `need` doubles: grows, never shrinks.  A new block takes the sticky pivot flag with it (nr_info points
// into the block); `lowrank`: ... and starts zeroed, for the low-rank solves, whose flag lives at its end.
int ensure_solve_workspace(prg_cpd* h, size_t need, bool lowrank);
// Waits for the stream, reads the flag and fails with "<who>: S is not positive definite at pivot <p><hint>" if it is set.
int report_pivot(prg_cpd* h, const int* info, const char* who, const char* hint = "");
}  // namespace prg
