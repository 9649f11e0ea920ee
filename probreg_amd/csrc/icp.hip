// ICP: Open3D's registration_icp, point-to-point and point-to-plane, and generalized ICP (plane-to-plane,
// DESIGN.md 3.16), on the cross-cloud search of grid_search.hip.  This file is the plan's lifecycle, its clouds and pose, and
// what a step is made of.  All in fp64 with fixed-order sums and no floating-point atomics.
//
//   sums     one lane per run of kRun consecutive source points (ascending m), a workgroup of kSlots lanes adds the runs in
//            ascending order and finishes: count, sum of d2, the stop test, the centroids.
//   step     one lane: Kabsch (kabsch_pose.h) or the 6 x 6 Cholesky solve, then the pose update.
//   gicp     a covariance per point (6 doubles, given or from a unit normal in closed form); per matched pair the 3 x 3
//            M = C_target + R C_source R^T is inverted by its adjugate and weights the pair's 6 x 6 system (MODE 3 of the sums).
// The loop "search, sums, step" stays on the device: its state (pose, stop flag, counters) is a device array, every kernel
// returns at once when the stop flag is set, and the host looks at the flag once per chunk of iterations.
//
// Every decision value is computed with separately rounded multiplications and additions (no contraction into FMAs), so that
// a restatement in plain IEEE arithmetic takes the same branches and gets the same sums.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "icp_plan.h"
#include "kabsch_pose.h"
#include "pose_step.h"

using namespace prg::icp;
using prg::cholesky6;
using prg::kPivot;

namespace {

constexpr int kStatusOk = 0, kStatusTooFew = 1, kStatusDegenerate = 2;
constexpr int kPointToPoint = 0, kPointToPlane = 1, kGeneralized = 2;
constexpr int kCov = 6;  // doubles per covariance: xx, xy, xz, yy, yz, zz

// ----------------------------------------------------------------------------------------------------------------- sums
// One run of kRun source points per lane, ascending m, matched points only; the target point and its normal are read by
// their index.  part: [run][kSlots].
//   MODE 0  (count, sum d2, sum q (3), sum y (3))                          point-to-point, first pass
//   MODE 1  (q - qm)_a (y - ym)_b, a major (9)                              point-to-point, second pass
//   MODE 2  (count, sum d2, J J^T upper triangle row-major (21), J res (6)) point-to-plane; J = (q x n, n), res = n . (q - y)
//   MODE 3  (count, sum d2, J^T P J upper triangle row-major (21), J^T P d (6), d^T P d) generalized; J = (-[q]x | I),
//           d = q - y, P the inverse of C_target + R C_source R^T (cs, ct: kCov doubles per source / target point)
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_icp_sums(const double* __restrict__ src, int64_t M, const double4* __restrict__ tp,
                                                     const double4* __restrict__ tn, const double* __restrict__ cs,
                                                     const double* __restrict__ ct, const int* __restrict__ idx,
                                                     const double* __restrict__ d2, const double* __restrict__ state,
                                                     double* __restrict__ part) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t m0 = r * kRun;
    if (m0 >= M || state[kStStop] != 0.0) return;
    const int64_t m1 = m0 + kRun < M ? m0 + kRun : M;
    double pose[12], ctr[6], acc[kSlots];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = state[kStPose + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) ctr[k] = state[kStCentre + k];
#pragma unroll
    for (int k = 0; k < kSlots; ++k) acc[k] = 0.0;
    for (int64_t m = m0; m < m1; ++m) {
        const int t = idx[m];
        if (t < 0) continue;
        double q[3];
        moved(pose, src + m * 3, q);
        const double4 y4 = tp[t];
        const double y[3] = {y4.x, y4.y, y4.z};
        if (MODE == 0) {
            acc[0] += 1.0;
            acc[1] += d2[m];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[2 + a] += q[a];
                acc[5 + a] += y[a];
            }
        } else if (MODE == 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[3 * a + b] += (q[a] - ctr[a]) * (y[b] - ctr[3 + b]);
        } else if (MODE == 3) {
            const double* __restrict__ a = cs + m * kCov;
            const double* __restrict__ b = ct + (int64_t)t * kCov;
            const double c[3][3] = {{a[0], a[1], a[2]}, {a[1], a[3], a[4]}, {a[2], a[4], a[5]}};
            double rc[3][3];  // R C_source
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    rc[i][j] = (pose[3 * i] * c[0][j] + pose[3 * i + 1] * c[1][j]) + pose[3 * i + 2] * c[2][j];
            double mm[6];  // M = C_target + (R C_source) R^T, upper triangle
            int s = 0;
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = i; j < 3; ++j, ++s)
                    mm[s] = b[s] + ((rc[i][0] * pose[3 * j] + rc[i][1] * pose[3 * j + 1]) + rc[i][2] * pose[3 * j + 2]);
            // P = adj(M) / det(M)
            const double c00 = mm[3] * mm[5] - mm[4] * mm[4], c01 = mm[2] * mm[4] - mm[1] * mm[5];
            const double c02 = mm[1] * mm[4] - mm[2] * mm[3], c11 = mm[0] * mm[5] - mm[2] * mm[2];
            const double c12 = mm[1] * mm[2] - mm[0] * mm[4], c22 = mm[0] * mm[3] - mm[1] * mm[1];
            const double det = (mm[0] * c00 + mm[1] * c01) + mm[2] * c02;
            const double p01 = c01 / det, p02 = c02 / det, p12 = c12 / det;
            const double P[3][3] = {{c00 / det, p01, p02}, {p01, c11 / det, p12}, {p02, p12, c22 / det}};
            const double d[3] = {q[0] - y[0], q[1] - y[1], q[2] - y[2]};
            double B[3][3], E[3][3], v[3];  // B = P (-[q]x): row a is q x P_a;  E = (-[q]x)^T B;  v = P d
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                B[i][0] = q[1] * P[i][2] - q[2] * P[i][1];
                B[i][1] = q[2] * P[i][0] - q[0] * P[i][2];
                B[i][2] = q[0] * P[i][1] - q[1] * P[i][0];
                v[i] = (P[i][0] * d[0] + P[i][1] * d[1]) + P[i][2] * d[2];
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                E[0][j] = q[1] * B[2][j] - q[2] * B[1][j];
                E[1][j] = q[2] * B[0][j] - q[0] * B[2][j];
                E[2][j] = q[0] * B[1][j] - q[1] * B[0][j];
            }
            acc[0] += 1.0;
            acc[1] += d2[m];
            s = 2;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = i; j < 3; ++j) acc[s++] += E[i][j];
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[s++] += B[j][i];
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = i; j < 3; ++j) acc[s++] += P[i][j];
            acc[23] += q[1] * v[2] - q[2] * v[1];
            acc[24] += q[2] * v[0] - q[0] * v[2];
            acc[25] += q[0] * v[1] - q[1] * v[0];
#pragma unroll
            for (int i = 0; i < 3; ++i) acc[26 + i] += v[i];
            acc[29] += (d[0] * v[0] + d[1] * v[1]) + d[2] * v[2];
        } else {
            const double4 n4 = tn[t];
            const double n[3] = {n4.x, n4.y, n4.z};
            const double res = (n[0] * (q[0] - y[0]) + n[1] * (q[1] - y[1])) + n[2] * (q[2] - y[2]);
            const double J[6] = {q[1] * n[2] - q[2] * n[1], q[2] * n[0] - q[0] * n[2], q[0] * n[1] - q[1] * n[0],
                                 n[0], n[1], n[2]};
            acc[0] += 1.0;
            acc[1] += d2[m];
            int s = 2;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) acc[s++] += J[i] * J[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[23 + i] += J[i] * res;
        }
    }
#pragma unroll
    for (int k = 0; k < kSlots; ++k) part[r * kSlots + k] = acc[k];
}

// One workgroup of kSlots lanes: lane k adds slot k of the runs in ascending run order and keeps the total in the state
// (mode 1: kStSumsB, else kStSumsA).  Modes 0, 2 and 3 are also the evaluation of the current pose: count, sum, fitness,
// rmse - and, with `test`, Open3D's stop test against the evaluation before.  Mode 0 leaves the centroids for the second pass.
__global__ __launch_bounds__(kSlots) void k_icp_finish(const double* __restrict__ part, int64_t nruns, int mode, int test,
                                                       double m_total, double rel_fitness, double rel_rmse,
                                                       double* __restrict__ state) {
    __shared__ double tot[kSlots];
    if (state[kStStop] != 0.0) return;
    double acc = 0.0;
    int64_t r = 0;
    for (; r + 16 <= nruns; r += 16) {  // sixteen loads in flight; the additions stay in ascending run order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = part[(r + u) * kSlots + threadIdx.x];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; r < nruns; ++r) acc += part[r * kSlots + threadIdx.x];
    tot[threadIdx.x] = acc;
    state[(mode == 1 ? kStSumsB : kStSumsA) + threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0 || mode == 1) return;
    const double cnt = tot[0];
    const double fitness = cnt / m_total;
    const double rmse = cnt > 0.0 ? sqrt(tot[1] / cnt) : 0.0;
    if (test) {
        if (state[kStEvals] > 0.0 && fabs(fitness - state[kStFitness]) < rel_fitness &&
            fabs(rmse - state[kStRmse]) < rel_rmse) {
            state[kStStop] = 1.0;
            state[kStConverged] = 1.0;
        }
        state[kStEvals] += 1.0;
    }
    state[kStCount] = cnt;
    state[kStSum] = tot[1];
    state[kStFitness] = fitness;
    state[kStRmse] = rmse;
    if (mode == 0)
        for (int k = 0; k < 6; ++k) state[kStCentre + k] = cnt > 0.0 ? tot[2 + k] / cnt : 0.0;
}

// ---------------------------------------------------------------------------------------------------------- covariances
// C = I - (1 - eps) u u^T of the unit normal u = n / |n| (Open3D's R diag(eps, 1, 1) R^T without the rotation): kCov doubles
// per point.  The host has checked that every |n| is finite and > 0.
__global__ __launch_bounds__(kBlock) void k_icp_cov_from_normals(const double* __restrict__ nrm, int64_t n, double eps,
                                                                 double* __restrict__ cov) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double n0 = nrm[i * 3], n1 = nrm[i * 3 + 1], n2 = nrm[i * 3 + 2];
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    const double u[3] = {n0 / len, n1 / len, n2 / len};
    const double k = 1.0 - eps;
    const double w[3] = {k * u[0], k * u[1], k * u[2]};
    double* __restrict__ c = cov + i * kCov;
    c[0] = 1.0 - w[0] * u[0];
    c[1] = -(w[0] * u[1]);
    c[2] = -(w[0] * u[2]);
    c[3] = 1.0 - w[1] * u[1];
    c[4] = -(w[1] * u[2]);
    c[5] = 1.0 - w[2] * u[2];
}

// ----------------------------------------------------------------------------------------------------------------- step
// One lane.  The step from the sums in the state; a missing step (too few matches, degenerate) sets the stop flag and the
// status and leaves the pose as it is.  R <- dR R, t <- dR t + dt.
__global__ void k_icp_step(int kind, double* __restrict__ state) {
    if (threadIdx.x != 0 || state[kStStop] != 0.0) return;
    const double cnt = state[kStCount];
    double d[12];
    if (kind == kPointToPoint) {
        if (cnt < 3.0) {
            state[kStStop] = 1.0;
            state[kStStatus] = (double)kStatusTooFew;
            return;
        }
        double hm[3][3], qm[3], ym[3];
        for (int a = 0; a < 3; ++a) {
            qm[a] = state[kStCentre + a];
            ym[a] = state[kStCentre + 3 + a];
            for (int b = 0; b < 3; ++b) hm[a][b] = state[kStSumsB + 3 * a + b];
        }
        prg::kabsch_pose(hm, qm, ym, d);
    } else {
        double x[6];
        if (cnt < 6.0 || !cholesky6(state + kStSumsA + 2, state + kStSumsA + 23, x)) {
            state[kStStop] = 1.0;
            state[kStStatus] = (double)kStatusDegenerate;
            return;
        }
        prg::twist_to_pose(x, d);  // Open3D's TransformVector6dToMatrix4d
    }
    prg::compose_pose(d, state + kStPose);
    state[kStIter] += 1.0;
}

// clears the stop flag and the status; `loop`: the counters of a loop as well
__global__ void k_icp_reset(int loop, double* __restrict__ state) {
    if (threadIdx.x != 0) return;
    state[kStStop] = 0.0;
    state[kStStatus] = (double)kStatusOk;
    if (loop) {
        state[kStIter] = 0.0;
        state[kStConverged] = 0.0;
        state[kStEvals] = 0.0;
    }
}

int check_kind(const char* who, prg_icp* h, int kind) {
    PRG_REQUIRE(kind == kPointToPoint || kind == kPointToPlane || kind == kGeneralized, PRG_ERR_INVALID,
                "%s: kind must be 0 (point-to-point), 1 (point-to-plane) or 2 (generalized), got %d", who, kind);
    PRG_REQUIRE(kind != kPointToPlane || h->have_normals, PRG_ERR_STATE,
                "%s: point-to-plane needs the target's normals (prg_icp_set_target)", who);
    PRG_REQUIRE(kind != kGeneralized || (h->have_cov[0] && h->have_cov[1]), PRG_ERR_STATE,
                "%s: generalized ICP needs the covariances of the %s (prg_icp_set_covariances or "
                "prg_icp_set_covariances_from_normals, after the cloud is set)", who,
                h->have_cov[0] ? "target" : (h->have_cov[1] ? "source" : "source and of the target"));
    return PRG_OK;
}

// the cloud `which` (0 source, 1 target) is set and has n points
int cov_rows(prg_icp* h, const char* who, int which, int64_t n, int64_t* rows) {
    PRG_REQUIRE(which == 0 || which == 1, PRG_ERR_INVALID, "%s: which must be 0 (source) or 1 (target), got %d", who, which);
    *rows = which == 0 ? h->M : h->N;
    PRG_REQUIRE(*rows >= 1, PRG_ERR_STATE, "%s: no %s (prg_icp_set_%s first)", who, which == 0 ? "source" : "target",
                which == 0 ? "source" : "target");
    PRG_REQUIRE(n == *rows, PRG_ERR_INVALID, "%s: need one row per %s point (%lld), got %lld", who,
                which == 0 ? "source" : "target", (long long)*rows, (long long)n);
    return PRG_OK;
}

// the pivot rule of cholesky6 on a 3 x 3 covariance (xx, xy, xz, yy, yz, zz)
bool positive_definite3(const double* c) {
    const double floor_ = kPivot * std::max(c[0], std::max(c[3], c[5]));
    const double d0 = c[0];
    if (!(d0 > floor_)) return false;
    const double l00 = std::sqrt(d0), l10 = c[1] / l00, l20 = c[2] / l00;
    const double d1 = c[3] - l10 * l10;
    if (!(d1 > floor_)) return false;
    const double l11 = std::sqrt(d1), l21 = (c[4] - l20 * l10) / l11;
    const double d2 = (c[5] - l20 * l20) - l21 * l21;
    return d2 > floor_;
}

int ensure_state(prg_icp* h) {
    if (h->state.p) return PRG_OK;
    PRG_HIP(h->state.reset(kStLen));
    double init[kStLen] = {0.0};
    init[0] = init[4] = init[8] = 1.0;
    PRG_HIP(hipMemcpy(h->state.p, init, sizeof(init), hipMemcpyHostToDevice));
    return PRG_OK;
}

template <int MODE>
void enqueue_sums(prg_icp* h, int test, double rel_fitness, double rel_rmse) {
    const int64_t nruns = prg::ceil_div(h->M, kRun);
    k_icp_sums<MODE><<<(unsigned)prg::ceil_div(nruns, kBlock), kBlock, 0, h->stream>>>(h->src.p, h->M, h->tp.p, h->tn.p, h->cov[0].p,
                                                                                     h->cov[1].p, h->idx.p, h->d2.p, h->state.p,
                                                                                     h->part.p);
    k_icp_finish<<<1, kSlots, 0, h->stream>>>(h->part.p, nruns, MODE, test, (double)h->M, rel_fitness, rel_rmse, h->state.p);
}

// the sums of the current matches that evaluate the pose and start a step of `kind`
void enqueue_eval(prg_icp* h, int kind, int test, double rel_fitness, double rel_rmse) {
    if (kind == kPointToPoint) enqueue_sums<0>(h, test, rel_fitness, rel_rmse);
    else if (kind == kPointToPlane) enqueue_sums<2>(h, test, rel_fitness, rel_rmse);
    else enqueue_sums<3>(h, test, rel_fitness, rel_rmse);
}

// the step itself, from the sums of enqueue_eval
void enqueue_step(prg_icp* h, int kind) {
    if (kind == kPointToPoint) enqueue_sums<1>(h, 0, 0.0, 0.0);
    k_icp_step<<<1, 1, 0, h->stream>>>(kind, h->state.p);
}

}  // namespace

namespace prg {
namespace icp {

int require_ready(prg_icp* h, const char* who, bool matches) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "%s: NULL argument", who);
    PRG_REQUIRE(h->N >= 1, PRG_ERR_STATE, "%s: no target (prg_icp_set_target first)", who);
    PRG_REQUIRE(h->M >= 1, PRG_ERR_STATE, "%s: no source (prg_icp_set_source first)", who);
    PRG_REQUIRE(!matches || h->have_matches, PRG_ERR_STATE, "%s: no matches (prg_icp_search first)", who);
    return PRG_OK;
}

void drop_lists(prg_icp* h) {
    h->have_knn = 0;
    h->have_counts = false;
    h->have_outlier = 0;
    h->have_dbscan = false;
}

}  // namespace icp
}  // namespace prg

extern "C" {

int prg_icp_create(prg_icp** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_icp_destroy(prg_icp* h) {
    return prg::destroy_handle(h);
}

int prg_icp_set_target(prg_icp* h, const double* points_hd, const double* normals_hd, int64_t n, double cell_edge) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_icp_set_target: NULL argument");
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_icp_set_target: need 1 <= n < 2^31 points, got %lld",
                (long long)n);
    PRG_REQUIRE(cell_edge >= 0.0 && std::isfinite(cell_edge), PRG_ERR_INVALID,
                "prg_icp_set_target: cell_edge must be finite and >= 0 (0: chosen from the cloud), got %g", cell_edge);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->N = 0;
    h->have_normals = h->have_order = h->have_matches = h->have_cov[1] = false;
    drop_lists(h);
    std::vector<double> raw, pad;
    double lo[3], hi[3];
    PRG_TRY(prg::load_cloud3(points_hd, n, 3, "prg_icp_set_target: the points contain NaN or infinity", raw, pad, lo, hi));
    PRG_HIP(h->tp.ensure(n, n));
    PRG_HIP(hipMemcpy(h->tp.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
    PRG_TRY(build_levels(h, raw, n, lo, hi, cell_edge));
    if (normals_hd) {
        PRG_TRY(prg::load_cloud3(normals_hd, n, 3, "prg_icp_set_target: the normals contain NaN or infinity", raw, pad, nullptr,
                                 nullptr));
        PRG_HIP(h->tn.ensure(n, n));
        PRG_HIP(hipMemcpy(h->tn.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    PRG_TRY(ensure_state(h));
    h->N = n;
    h->have_normals = normals_hd != nullptr;
    return PRG_OK;
}

int prg_icp_set_source(prg_icp* h, const double* points_hd, int64_t m) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_icp_set_source: NULL argument");
    PRG_REQUIRE(m >= 1 && m < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_icp_set_source: need 1 <= m < 2^31 points, got %lld",
                (long long)m);
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->M = 0;
    h->have_order = h->have_matches = h->have_cov[0] = false;
    drop_lists(h);
    std::vector<double> raw((size_t)m * 3);
    PRG_HIP(hipMemcpy(raw.data(), points_hd, raw.size() * sizeof(double), hipMemcpyDefault));
    for (size_t i = 0; i < raw.size(); ++i)
        PRG_REQUIRE(std::isfinite(raw[i]), PRG_ERR_INVALID, "prg_icp_set_source: the points contain NaN or infinity");
    const int64_t nruns = prg::ceil_div(m, kRun);
    PRG_HIP(h->src.ensure(m * 3, m * 3));
    PRG_HIP(h->qkeys.ensure(2 * m, 2 * m));
    PRG_HIP(h->qvals.ensure(2 * m, 2 * m));
    PRG_HIP(h->idx.ensure(m, m));
    PRG_HIP(h->d2.ensure(m, m));
    PRG_HIP(h->part.ensure(nruns * kSlots, nruns * kSlots));
    PRG_HIP(hipMemcpy(h->src.p, raw.data(), raw.size() * sizeof(double), hipMemcpyHostToDevice));
    PRG_TRY(ensure_state(h));
    h->M = m;
    return PRG_OK;
}

int prg_icp_set_covariances(prg_icp* h, int which, const double* cov_hd, int64_t n) {
    PRG_REQUIRE(h && cov_hd, PRG_ERR_INVALID, "prg_icp_set_covariances: NULL argument");
    int64_t rows = 0;
    PRG_TRY(cov_rows(h, "prg_icp_set_covariances", which, n, &rows));
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_cov[which] = false;
    std::vector<double> raw((size_t)rows * kCov);
    PRG_HIP(hipMemcpy(raw.data(), cov_hd, raw.size() * sizeof(double), hipMemcpyDefault));
    for (int64_t i = 0; i < rows; ++i) {
        const double* c = raw.data() + (size_t)i * kCov;
        for (int k = 0; k < kCov; ++k)
            PRG_REQUIRE(std::isfinite(c[k]), PRG_ERR_INVALID, "prg_icp_set_covariances: the covariances contain NaN or infinity");
        PRG_REQUIRE(positive_definite3(c), PRG_ERR_INVALID,
                    "prg_icp_set_covariances: covariance %lld is not positive definite (a Cholesky pivot <= 1e-12 max diag)",
                    (long long)i);
    }
    PRG_HIP(h->cov[which].ensure(rows * kCov, rows * kCov));
    PRG_HIP(hipMemcpy(h->cov[which].p, raw.data(), raw.size() * sizeof(double), hipMemcpyHostToDevice));
    h->have_cov[which] = true;
    return PRG_OK;
}

int prg_icp_set_covariances_from_normals(prg_icp* h, int which, const double* normals_hd, int64_t n, double epsilon) {
    PRG_REQUIRE(h && normals_hd, PRG_ERR_INVALID, "prg_icp_set_covariances_from_normals: NULL argument");
    int64_t rows = 0;
    PRG_TRY(cov_rows(h, "prg_icp_set_covariances_from_normals", which, n, &rows));
    PRG_REQUIRE(epsilon > 0.0 && epsilon <= 1.0, PRG_ERR_INVALID,
                "prg_icp_set_covariances_from_normals: epsilon must lie in (0, 1], got %g", epsilon);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->have_cov[which] = false;
    std::vector<double> raw((size_t)rows * 3);
    PRG_HIP(hipMemcpy(raw.data(), normals_hd, raw.size() * sizeof(double), hipMemcpyDefault));
    for (int64_t i = 0; i < rows; ++i) {
        const double* v = raw.data() + (size_t)i * 3;
        const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);  // NaN for a NaN entry
        PRG_REQUIRE(std::isfinite(len) && len > 0.0, PRG_ERR_INVALID,
                    "prg_icp_set_covariances_from_normals: normal %lld has no finite length > 0", (long long)i);
    }
    prg::DevBuf<double> nrm;
    PRG_HIP(nrm.reset(rows * 3));
    PRG_HIP(h->cov[which].ensure(rows * kCov, rows * kCov));
    PRG_HIP(hipMemcpy(nrm.p, raw.data(), raw.size() * sizeof(double), hipMemcpyHostToDevice));
    k_icp_cov_from_normals<<<(unsigned)prg::ceil_div(rows, kBlock), kBlock, 0, st>>>(nrm.p, rows, epsilon, h->cov[which].p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(st));  // the normals go away with this scope
    h->have_cov[which] = true;
    return PRG_OK;
}

int prg_icp_get_covariances(prg_icp* h, int which, double* cov_host) {
    PRG_REQUIRE(h && cov_host, PRG_ERR_INVALID, "prg_icp_get_covariances: NULL argument");
    PRG_REQUIRE(which == 0 || which == 1, PRG_ERR_INVALID, "prg_icp_get_covariances: which must be 0 (source) or 1 (target), got %d",
                which);
    PRG_REQUIRE(h->have_cov[which], PRG_ERR_STATE, "prg_icp_get_covariances: the %s has no covariances",
                which == 0 ? "source" : "target");
    PRG_ENTER(h->device);
    return prg::copy_out(cov_host, h->cov[which], (which == 0 ? h->M : h->N) * kCov, h->stream);
}

int prg_icp_set_pose(prg_icp* h, const double* pose_host) {
    PRG_REQUIRE(h && pose_host, PRG_ERR_INVALID, "prg_icp_set_pose: NULL argument");
    for (int k = 0; k < 12; ++k)
        PRG_REQUIRE(std::isfinite(pose_host[k]), PRG_ERR_INVALID, "prg_icp_set_pose: the pose contains NaN or infinity");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_state(h));
    PRG_TRY(prg::copy_in(h->state, pose_host, 12, h->stream, kStPose));
    h->have_matches = false;
    drop_lists(h);
    return PRG_OK;
}

int prg_icp_get_pose(prg_icp* h, double* pose_host) {
    PRG_REQUIRE(h && pose_host, PRG_ERR_INVALID, "prg_icp_get_pose: NULL argument");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_state(h));
    PRG_TRY(prg::copy_out(pose_host, h->state, 12, h->stream, kStPose));
    return PRG_OK;
}

int prg_icp_search(prg_icp* h, double r) {
    PRG_TRY(require_ready(h, "prg_icp_search", false));
    PRG_REQUIRE(r > 0.0, PRG_ERR_INVALID, "prg_icp_search: r must be > 0 (infinity: no limit), got %g", r);
    PRG_ENTER(h->device);
    PRG_TRY(ensure_order(h));
    k_icp_reset<<<1, 1, 0, h->stream>>>(0, h->state.p);
    enqueue_search(h, r);
    PRG_HIP(hipGetLastError());
    h->have_matches = true;
    return PRG_OK;
}

int prg_icp_sums(prg_icp* h, int kind, double* out_host) {
    PRG_TRY(require_ready(h, "prg_icp_sums", true));
    PRG_REQUIRE(out_host != nullptr, PRG_ERR_INVALID, "prg_icp_sums: NULL argument");
    PRG_TRY(check_kind("prg_icp_sums", h, kind));
    PRG_ENTER(h->device);
    k_icp_reset<<<1, 1, 0, h->stream>>>(0, h->state.p);
    enqueue_eval(h, kind, 0, 0.0, 0.0);
    if (kind == kPointToPoint) enqueue_sums<1>(h, 0, 0.0, 0.0);
    PRG_HIP(hipGetLastError());
    double sums[2 * kSlots];
    PRG_HIP(hipMemcpyAsync(sums, h->state.p + kStSumsA, sizeof(sums), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    for (int k = 0; k < kSlots; ++k) out_host[k] = 0.0;
    if (kind == kPointToPoint) {
        for (int k = 0; k < 8; ++k) out_host[k] = sums[k];
        for (int k = 0; k < 9; ++k) out_host[8 + k] = sums[kSlots + k];
    } else {
        for (int k = 0; k < (kind == kGeneralized ? 30 : 29); ++k) out_host[k] = sums[k];
    }
    return PRG_OK;
}

int prg_icp_step(prg_icp* h, int kind) {
    PRG_TRY(require_ready(h, "prg_icp_step", true));
    PRG_TRY(check_kind("prg_icp_step", h, kind));
    PRG_ENTER(h->device);
    k_icp_reset<<<1, 1, 0, h->stream>>>(1, h->state.p);
    enqueue_eval(h, kind, 0, 0.0, 0.0);
    enqueue_step(h, kind);
    PRG_HIP(hipGetLastError());
    h->have_matches = false;  // they belong to the pose before the step
    drop_lists(h);
    return PRG_OK;
}

int prg_icp_iterate(prg_icp* h, int kind, double r, int max_iteration, double rel_fitness, double rel_rmse, int chunk) {
    PRG_TRY(require_ready(h, "prg_icp_iterate", false));
    PRG_TRY(check_kind("prg_icp_iterate", h, kind));
    PRG_REQUIRE(r > 0.0, PRG_ERR_INVALID, "prg_icp_iterate: r must be > 0 (infinity: no limit), got %g", r);
    PRG_REQUIRE(max_iteration >= 0 && max_iteration <= 1000000, PRG_ERR_INVALID,
                "prg_icp_iterate: max_iteration must lie in 0 .. 1000000, got %d", max_iteration);
    PRG_REQUIRE(std::isfinite(rel_fitness) && std::isfinite(rel_rmse), PRG_ERR_INVALID,
                "prg_icp_iterate: relative_fitness and relative_rmse must be finite");
    PRG_REQUIRE(chunk >= 1, PRG_ERR_INVALID, "prg_icp_iterate: chunk must be >= 1, got %d", chunk);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_TRY(ensure_order(h));
    drop_lists(h);  // the loop moves the pose
    k_icp_reset<<<1, 1, 0, st>>>(1, h->state.p);
    enqueue_search(h, r);
    enqueue_eval(h, kind, 1, rel_fitness, rel_rmse);
    PRG_HIP(hipGetLastError());
    h->have_matches = true;
    for (int done = 0; done < max_iteration;) {
        const int c = std::min(chunk, max_iteration - done);
        for (int i = 0; i < c; ++i) {
            enqueue_step(h, kind);
            enqueue_search(h, r);
            enqueue_eval(h, kind, 1, rel_fitness, rel_rmse);
        }
        PRG_HIP(hipGetLastError());
        done += c;
        double stop = 0.0;
        PRG_HIP(hipMemcpyAsync(&stop, h->state.p + kStStop, sizeof(double), hipMemcpyDeviceToHost, st));
        PRG_HIP(hipStreamSynchronize(st));
        if (stop != 0.0) break;
    }
    return PRG_OK;
}

int prg_icp_get_state(prg_icp* h, double* pose_host, int64_t* count_host, double* sum_host, int* n_iter_host,
                      int* converged_host, int* status_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_icp_get_state: NULL argument");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_state(h));
    double s[kStLen];
    PRG_TRY(prg::copy_out(s, h->state, kStLen, h->stream));
    if (pose_host)
        for (int k = 0; k < 12; ++k) pose_host[k] = s[kStPose + k];
    if (count_host) *count_host = (int64_t)s[kStCount];
    if (sum_host) *sum_host = s[kStSum];
    if (n_iter_host) *n_iter_host = (int)s[kStIter];
    if (converged_host) *converged_host = (int)s[kStConverged];
    if (status_host) *status_host = (int)s[kStStatus];
    return PRG_OK;
}

}  // extern "C"
