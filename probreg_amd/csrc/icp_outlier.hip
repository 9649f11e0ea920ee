// The two outlier filters of the ICP plan on the k-NN lists and the radius counts of grid_search.hip: the
// statistical one keeps a point whose mean neighbour distance is at most mu + std_ratio s, the radius one a point with more
// than nb_points neighbours.  fp64, every sum in a fixed order (runs of kRun, then the runs ascending), no FMA contraction.
#pragma clang fp contract(off)
#include <math.h>

#include <cmath>

#include "icp_plan.h"

using namespace prg::icp;

namespace {

constexpr int kOutMean = 0, kOutDev = 1, kOutThr = 2, kOutLen = 4;  // stat: mu, s, thr

// a_i = (sum of sqrt(d2) over the list, in list order from 0.0) / its length
__global__ __launch_bounds__(kBlock) void k_knn_mean_distance(const double* __restrict__ d2, const int* __restrict__ cnt, int k,
                                                              int64_t M, double* __restrict__ a) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const int len = cnt[i];
    double acc = 0.0;
    for (int t = 0; t < len; ++t) acc += sqrt(d2[i * k + t]);
    a[i] = len > 0 ? acc / (double)len : 0.0;
}

// One run of kRun consecutive i per lane, ascending from 0.0: a_i (dev 0) or (a_i - mu) (a_i - mu) (dev 1).  part: [run]
__global__ __launch_bounds__(kBlock) void k_outlier_runs(const double* __restrict__ a, int64_t M, int dev,
                                                         const double* __restrict__ stat, double* __restrict__ part) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i0 = r * kRun;
    if (i0 >= M) return;
    const int64_t i1 = i0 + kRun < M ? i0 + kRun : M;
    const double mu = dev ? stat[kOutMean] : 0.0;
    double acc = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        const double e = a[i] - mu;
        acc += dev ? e * e : a[i];
    }
    part[r] = acc;
}

// One lane: the run sums in ascending run order from 0.0, then mu = sum / M (dev 0), or s = sqrt(sum / (M - 1)), 0 when
// M = 1, and thr = mu + (std_ratio s) (dev 1).
__global__ void k_outlier_finish(const double* __restrict__ part, int64_t nruns, int dev, double m_total, double std_ratio,
                                 double* __restrict__ stat) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double acc = 0.0;
    int64_t r = 0;
    for (; r + 16 <= nruns; r += 16) {  // sixteen loads in flight; the additions stay in ascending run order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = part[r + u];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += v[u];
    }
    for (; r < nruns; ++r) acc += part[r];
    if (!dev) {
        stat[kOutMean] = acc / m_total;
        return;
    }
    const double s = m_total > 1.0 ? sqrt(acc / (m_total - 1.0)) : 0.0;
    const double scaled = std_ratio * s;
    stat[kOutDev] = s;
    stat[kOutThr] = stat[kOutMean] + scaled;
}

// keep i iff a_i <= thr
__global__ __launch_bounds__(kBlock) void k_outlier_mask_score(const double* __restrict__ a, int64_t M,
                                                               const double* __restrict__ stat, unsigned char* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < M) keep[i] = a[i] <= stat[kOutThr] ? 1 : 0;
}

// keep i iff c_i > nb_points
__global__ __launch_bounds__(kBlock) void k_outlier_mask_count(const int* __restrict__ c, int64_t M, int nb_points,
                                                               unsigned char* __restrict__ keep) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < M) keep[i] = c[i] > nb_points ? 1 : 0;
}

}  // namespace

extern "C" {

int prg_icp_outlier_statistical(prg_icp* h, int k, double std_ratio) {
    PRG_TRY(require_ready(h, "prg_icp_outlier_statistical", false));
    PRG_REQUIRE(std_ratio >= 0.0 && std::isfinite(std_ratio), PRG_ERR_INVALID,
                "prg_icp_outlier_statistical: std_ratio must be finite and >= 0, got %g", std_ratio);
    PRG_ENTER(h->device);
    h->have_outlier = 0;
    PRG_TRY(run_knn(h, "prg_icp_outlier_statistical", k, INFINITY));
    const int64_t M = h->M, nruns = prg::ceil_div(M, kRun);  // part holds nruns kSlots doubles (prg_icp_set_source)
    PRG_HIP(h->score.ensure(M, M));
    PRG_HIP(h->keep.ensure(M, M));
    PRG_HIP(h->stat.ensure(kOutLen, kOutLen));
    hipStream_t st = h->stream;
    const unsigned blocks = (unsigned)prg::ceil_div(M, kBlock), run_blocks = (unsigned)prg::ceil_div(nruns, kBlock);
    k_knn_mean_distance<<<blocks, kBlock, 0, st>>>(h->knn_d2.p, h->knn_cnt.p, k, M, h->score.p);
    for (int dev = 0; dev < 2; ++dev) {
        k_outlier_runs<<<run_blocks, kBlock, 0, st>>>(h->score.p, M, dev, h->stat.p, h->part.p);
        k_outlier_finish<<<1, 1, 0, st>>>(h->part.p, nruns, dev, (double)M, std_ratio, h->stat.p);
    }
    k_outlier_mask_score<<<blocks, kBlock, 0, st>>>(h->score.p, M, h->stat.p, h->keep.p);
    PRG_HIP(hipGetLastError());
    h->have_outlier = 1;
    return PRG_OK;
}

int prg_icp_outlier_radius(prg_icp* h, double r, int nb_points) {
    PRG_TRY(require_ready(h, "prg_icp_outlier_radius", false));
    PRG_REQUIRE(nb_points >= 0, PRG_ERR_INVALID, "prg_icp_outlier_radius: nb_points must be >= 0, got %d", nb_points);
    PRG_ENTER(h->device);
    h->have_outlier = 0;
    PRG_TRY(run_radius_count(h, "prg_icp_outlier_radius", r));
    const int64_t M = h->M;
    PRG_HIP(h->keep.ensure(M, M));
    k_outlier_mask_count<<<(unsigned)prg::ceil_div(M, kBlock), kBlock, 0, h->stream>>>(h->counts.p, M, nb_points, h->keep.p);
    PRG_HIP(hipGetLastError());
    h->have_outlier = 2;
    return PRG_OK;
}

int prg_icp_get_outlier(prg_icp* h, unsigned char* keep_host, double* score_host, double* stat_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_outlier", false));
    PRG_REQUIRE(h->have_outlier != 0, PRG_ERR_STATE,
                "prg_icp_get_outlier: no filter result (prg_icp_outlier_statistical or prg_icp_outlier_radius first)");
    PRG_REQUIRE(h->have_outlier == 1 || (score_host == nullptr && stat_host == nullptr), PRG_ERR_STATE,
                "prg_icp_get_outlier: the radius filter has no score or statistics (its counts: prg_icp_get_counts)");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(keep_host, h->keep, h->M, h->stream));
    PRG_TRY(prg::copy_out(score_host, h->score, h->M, h->stream));
    PRG_TRY(prg::copy_out(stat_host, h->stat, 3, h->stream));
    return PRG_OK;
}

}  // extern "C"
