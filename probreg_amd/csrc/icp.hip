// ICP: Open3D's registration_icp, point-to-point and point-to-plane, on a cross-cloud grid search, and
// generalized ICP (plane-to-plane) on the same search, sums and loop.  All in fp64 with fixed-order sums and
// no floating-point atomics.
//
//   grid     the cell grid of cell_grid.h, built once per target.  The cell edge comes from the cloud (a few points per
//            occupied cell), never from the search radius.  Coarser levels (edge x kLevelStep each, until the box is one or
//            two cells wide - always reached, see floor_edge) are built the same way: they carry a query that is far from the cloud
//            over the empty space, and the last one bounds every search.
//   search   one query per lane, queries in Morton order of their moved position.  Shells of cells of growing Chebyshev
//            distance s around the query's clamped cell, kLevelShells of them per level and any number on the last level;
//            after shell s of a level with edge h everything unvisited is farther than
//            sqrt((s h)^2 + D^2), D the query's distance to the target's box.  The lane stops when its best d2 is strictly
//            below that bound (shrunk by a hair), when the bound exceeds r, or when every cell that meets the cube of half
//            edge min(r, sqrt(best d2)) around the query is visited (the shells are clipped to that cube).  The result is the
//            minimum of (d2, index) over the visited points, which does not depend on the order of the visits: the grid
//            does not show.
//   sums     one lane per run of kRun consecutive source points (ascending m), a workgroup of kSlots lanes adds the runs in
//            ascending order and finishes: count, sum of d2, the stop test, the centroids.
//   step     one lane: Kabsch (kabsch_pose.h) or the 6 x 6 Cholesky solve, then the pose update.
//   gicp     a covariance per point (6 doubles, given or from a unit normal in closed form); per matched pair the 3 x 3
//            M = C_target + R C_source R^T is inverted by its adjugate and weights the pair's 6 x 6 system (MODE 3 of the sums).
//   knn      the k best instead of the best: one wave per query, the sorted list one entry per lane, on the
//            same levels, shells, bound and clipping; a radius count; and the two outlier filters on top of them.
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

#include "cell_grid.h"
#include "dev_buf.h"
#include "kabsch_pose.h"
#include "lattice_sort.h"
#include "prg_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRun = 64;                   // source points per run of the ordered sums (part of the definition)
constexpr int kSlots = 32;                 // sums per run: 8 / 9 (point-to-point, two passes), 29 (point-to-plane), 30 (generalized)
constexpr double kReach = 1.0 + 1.0e-12;   // the stop bound is a hair smaller than (s h)^2 + D^2: covers the rounding of d2
constexpr int kOrderBits = 10;             // per axis, of the Morton key that orders the queries
constexpr double kPivot = 1.0e-12;         // a Cholesky pivot <= kPivot max diag(A) is degenerate (part of the definition)
constexpr int kSample = 16384;             // points that choose the cell edge
constexpr int kMaxLevels = 16;             // grids of growing cell edge: kLevelStep^(kMaxLevels - 1) = 2^kFloorBits
constexpr int kFloorBits = 30;             // no cell edge is below the largest extent / 2^kFloorBits
constexpr double kLevelStep = 4.0;         // edge of a level / edge of the level below
constexpr int kLevelShells = 2;            // shells 0 .. kLevelShells of a level are walked before the next level takes over

// state (doubles)
constexpr int kStPose = 0, kStCentre = 12, kStStop = 18, kStCount = 19, kStSum = 20, kStFitness = 21, kStRmse = 22,
              kStIter = 23, kStConverged = 24, kStStatus = 25, kStEvals = 26, kStSumsA = 32, kStSumsB = 64, kStLen = 96;
constexpr int kStatusOk = 0, kStatusTooFew = 1, kStatusDegenerate = 2;
constexpr int kPointToPoint = 0, kPointToPlane = 1, kGeneralized = 2;
constexpr int kCov = 6;  // doubles per covariance: xx, xy, xz, yy, yz, zz

using prg::CellGrid;
using prg::cell_key;
using prg::cell_of;

struct Levels {
    int count;
    CellGrid g[kMaxLevels];
    const double4* sp[kMaxLevels];  // the points in the cell order of the level, original index in .w
    const int2* cells[kMaxLevels];  // (begin, end) of every bucket
};

// q_a = ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) + t_a
__device__ __forceinline__ void moved(const double (&m)[12], const double* __restrict__ p, double (&q)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((m[3 * a] * p[0] + m[3 * a + 1] * p[1]) + m[3 * a + 2] * p[2]) + m[9 + a];
}

__device__ __forceinline__ unsigned spread10(unsigned v) {  // 10 bits -> every third bit
    v &= 0x3ffu;
    v = (v | v << 16) & 0x030000ffu;
    v = (v | v << 8) & 0x0300f00fu;
    v = (v | v << 4) & 0x030c30c3u;
    v = (v | v << 2) & 0x09249249u;
    return v;
}

// Morton key of the moved source point on a 2^kOrderBits grid over the target's box (clamped): orders the queries only
__global__ __launch_bounds__(kBlock) void k_icp_query_keys(const double* __restrict__ src, int64_t M,
                                                           const double* __restrict__ state, CellGrid g, double scale,
                                                           unsigned* __restrict__ keys, int* __restrict__ vals) {
    const int64_t m = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (m >= M) return;
    double pose[12], q[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = state[kStPose + k];
    moved(pose, src + m * 3, q);
    unsigned key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double c = floor((q[a] - g.lo[a]) * scale);
        c = c > 0.0 ? c : 0.0;
        c = c < (double)((1 << kOrderBits) - 1) ? c : (double)((1 << kOrderBits) - 1);
        key |= spread10((unsigned)c) << a;
    }
    keys[m] = key;
    vals[m] = (int)m;
}

// --------------------------------------------------------------------------------------------------------------- search
struct Best {
    double d2;
    int idx;
};

// every point of the bucket of cell (cx, cy, cz): d2 = (dx dx + dy dy) + dz dz, minimum of (d2, index)
__device__ __forceinline__ void visit(const double4* __restrict__ sp, const int2* __restrict__ cells, const CellGrid& g, int cx,
                                      int cy, int cz, const double (&q)[3], Best& b) {
    const int2 be = cells[cell_key(cx, cy, cz, g)];
    for (int t = be.x; t < be.y; ++t) {
        const double4 y = sp[t];
        const double dx = y.x - q[0], dy = y.y - q[1], dz = y.z - q[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const int idx = (int)y.w;
        if (b.idx < 0 || d2 < b.d2 || (d2 == b.d2 && idx < b.idx)) {
            b.d2 = d2;
            b.idx = idx;
        }
    }
}

// The shells of one level around the query, clipped to the cells that can hold a point at most rho = min(r, sqrt(best d2))
// (a hair more) from it: cell_of is monotone, so a point in a cell below lo[a] has y_a < q_a - rho and d2 > rho^2.  Returns
// true when the search is over: the best d2 is strictly below what anything unvisited can have, that bound exceeds r, or every
// cell that matters has been visited.  false: `shells` shells were not enough (never on the last level).
__device__ inline bool walk_level(const CellGrid& g, const double4* __restrict__ sp, const int2* __restrict__ cells,
                                  const double (&q)[3], double box2, double r2, int shells, double& rho, Best& b) {
    int c[3], lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = min(cell_of(q[a], g.lo[a], g.edge), g.dim[a] - 1);
    for (int s = 0;; ++s) {
        int smax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wide = rho + (fabs(q[a]) + rho) * 0x1p-50;  // the rounding of q_a -+ rho
            lo[a] = min(cell_of(q[a] - wide, g.lo[a], g.edge), g.dim[a] - 1);
            hi[a] = min(cell_of(q[a] + wide, g.lo[a], g.edge), g.dim[a] - 1);
            smax = max(smax, max(c[a] - lo[a], hi[a] - c[a]));
        }
        if (s > smax) return true;
        if (s > shells) return false;
        const int z0 = max(c[2] - s, lo[2]), z1 = min(c[2] + s, hi[2]);
        const int y0 = max(c[1] - s, lo[1]), y1 = min(c[1] + s, hi[1]);
        const int xl = c[0] - s, xh = c[0] + s;
        for (int z = z0; z <= z1; ++z) {
            const bool zf = z - c[2] == s || c[2] - z == s;
            for (int y = y0; y <= y1; ++y) {
                if (zf || y - c[1] == s || c[1] - y == s) {  // a face of the shell: the whole row
                    const int x1 = min(xh, hi[0]);
                    for (int x = max(xl, lo[0]); x <= x1; ++x) visit(sp, cells, g, x, y, z, q, b);
                } else {  // inside: the two ends of the row (s > 0 here)
                    if (xl >= lo[0]) visit(sp, cells, g, xl, y, z, q, b);
                    if (xh <= hi[0]) visit(sp, cells, g, xh, y, z, q, b);
                }
            }
        }
        // what is not visited yet lies in cells at Chebyshev distance > s of the clamped cell: farther than the bound
        const double reach = fmax((double)s - g.slack, 0.0) * g.edge / kReach;
        const double bound = reach * reach + box2;
        if ((b.idx >= 0 && b.d2 < bound) || bound > r2) return true;
        if (b.idx >= 0) rho = fmin(rho, sqrt(b.d2) * kReach);
    }
}

// Lane l serves source point qorder[l] and writes by that index: out_idx (-1: nothing within r) and out_d2 (+inf then).
// The level loop is uniform; a lane whose search is over sits the coarser levels out.
__global__ __launch_bounds__(kBlock) void k_icp_search(Levels lv, const double* __restrict__ src,
                                                       const int* __restrict__ qorder, int64_t M,
                                                       const double* __restrict__ state, double r, double r2,
                                                       int* __restrict__ out_idx, double* __restrict__ out_d2) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= M || state[kStStop] != 0.0) return;
    const int m = qorder[l];
    double pose[12], q[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = state[kStPose + k];
    moved(pose, src + (int64_t)m * 3, q);
    double box2 = 0.0;  // squared distance of the query to the target's box
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = lv.g[0].lo[a], hi = lv.g[0].hi[a];
        const double out = q[a] < lo ? lo - q[a] : (q[a] > hi ? q[a] - hi : 0.0);
        box2 += out * out;
    }
    box2 = box2 / kReach;
    Best b = {INFINITY, -1};
    double rho = r * kReach;
    bool done = false;
    for (int k = 0; k < lv.count; ++k)
        if (!done)
            done = walk_level(lv.g[k], lv.sp[k], lv.cells[k], q, box2, r2,
                              k + 1 < lv.count ? kLevelShells : 0x7fffffff, rho, b);
    const bool hit = b.idx >= 0 && b.d2 <= r2;
    out_idx[m] = hit ? b.idx : -1;
    out_d2[m] = hit ? b.d2 : INFINITY;
}

// ---------------------------------------------------------------------------------------------------- k nearest (3.17)
// The k smallest (d2, index) among d2 <= r r, ascending: one wave per query, entry t of the sorted list in lane t.  `cnt`,
// `kd2` and `kidx` (the last key of a full list: the pruning key) are the same in every lane.
constexpr int kWave = 64;
constexpr int kMaxK = kWave;   // one list entry per lane
constexpr int kCountSpan = 4;  // the radius count walks the finest level on which the cube around r spans <= kCountSpan + 1 cells an axis

struct KList {
    double d2;
    int idx;
    int cnt;
    double kd2;
    int kidx;
};

__device__ __forceinline__ bool key_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

// One candidate (the same values in every lane) into the wave's list.  A key that is in the list already is a second visit
// of that point - a coarser level after the hand-over, two cells of one hashed bucket - and is dropped: d2 of a point is the
// same bits on every visit, and the last key only shrinks, so a point that was once refused or pushed out stays out.
__device__ __forceinline__ void knn_insert(KList& b, int k, int lane, double cd2, int cidx) {
    const bool mine = lane < b.cnt;
    const unsigned long long below = __ballot(mine && key_less(b.d2, b.idx, cd2, cidx));
    const unsigned long long same = __ballot(mine && b.d2 == cd2 && b.idx == cidx);
    const int pos = __popcll(below);  // the list is sorted: `below` is its first pos lanes
    if (same != 0ull || pos >= k) return;
    const double ud2 = __shfl_up(b.d2, 1);
    const int uidx = __shfl_up(b.idx, 1);
    if (lane > pos) {
        b.d2 = ud2;
        b.idx = uidx;
    } else if (lane == pos) {
        b.d2 = cd2;
        b.idx = cidx;
    }
    b.cnt = min(b.cnt + 1, k);
}

// walk_level for a list.  The cells of the clipped shell are dealt to the lanes, every lane walks its bucket, and each round
// of one point per lane goes into the list in lane order.  The stop test and the clipping use the k-th d2, and only when the
// list is full; a shorter list ends by bound > r r or with the last cell that matters.  All control flow is wave-uniform.
__device__ inline bool knn_level(const CellGrid& g, const double4* __restrict__ sp, const int2* __restrict__ cells,
                                 const double (&q)[3], double box2, double r2, int shells, int k, int lane, double& rho,
                                 KList& b) {
    int c[3], lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = min(cell_of(q[a], g.lo[a], g.edge), g.dim[a] - 1);
    for (int s = 0;; ++s) {
        int smax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wide = rho + (fabs(q[a]) + rho) * 0x1p-50;  // the rounding of q_a -+ rho
            lo[a] = min(cell_of(q[a] - wide, g.lo[a], g.edge), g.dim[a] - 1);
            hi[a] = min(cell_of(q[a] + wide, g.lo[a], g.edge), g.dim[a] - 1);
            smax = max(smax, max(c[a] - lo[a], hi[a] - c[a]));
        }
        if (s > smax) return true;
        if (s > shells) return false;
        const int x0 = max(c[0] - s, lo[0]), y0 = max(c[1] - s, lo[1]), z0 = max(c[2] - s, lo[2]);
        const int nx = min(c[0] + s, hi[0]) - x0 + 1, ny = min(c[1] + s, hi[1]) - y0 + 1, nz = min(c[2] + s, hi[2]) - z0 + 1;
        // lo <= c <= hi: every extent is >= 1, and at most 2 s + 1 <= 5 - s <= kLevelShells below the last level, which is at
        // most two cells wide (run_knn checks it) - so the clipped cube has at most 125 cells and 32-bit arithmetic deals it.
        // Every shell enumerates the whole cube and leaves out the cells that are not at Chebyshev distance s: 35 of 125 at most.
        const int nxy = nx * ny, total = nxy * nz;
        for (int base = 0; base < total; base += kWave) {
            const int i = base + lane;
            int2 be = make_int2(0, 0);
            if (i < total) {
                const int z = z0 + i / nxy, y = y0 + (i % nxy) / nx, x = x0 + i % nx;
                if (max(abs(x - c[0]), max(abs(y - c[1]), abs(z - c[2]))) == s) be = cells[cell_key(x, y, z, g)];
            }
            for (int t = be.x; __ballot(t < be.y) != 0ull; ++t) {
                double d2 = INFINITY;
                int idx = 0x7fffffff;
                bool cand = false;
                if (t < be.y) {
                    const double4 y = sp[t];
                    const double dx = y.x - q[0], dy = y.y - q[1], dz = y.z - q[2];
                    d2 = (dx * dx + dy * dy) + dz * dz;
                    idx = (int)y.w;
                    cand = d2 <= r2 && (b.cnt < k || key_less(d2, idx, b.kd2, b.kidx));
                }
                for (unsigned long long todo = __ballot(cand); todo != 0ull; todo &= todo - 1ull) {
                    const int j = __builtin_ctzll(todo);
                    knn_insert(b, k, lane, __shfl(d2, j), __shfl(idx, j));
                }
                if (b.cnt == k) {
                    b.kd2 = __shfl(b.d2, k - 1);
                    b.kidx = __shfl(b.idx, k - 1);
                }
            }
        }
        // what is not visited yet lies in cells at Chebyshev distance > s of the clamped cell: farther than the bound
        const double reach = fmax((double)s - g.slack, 0.0) * g.edge / kReach;
        const double bound = reach * reach + box2;
        const bool full = b.cnt == k;
        if ((full && b.kd2 < bound) || bound > r2) return true;
        if (full) rho = fmin(rho, sqrt(b.kd2) * kReach);
    }
}

// Wave w serves source point qorder[w] and writes its k slots by that index: the list, then (-1, +inf); out_cnt its length.
__global__ __launch_bounds__(kBlock) void k_icp_knn(Levels lv, const double* __restrict__ src, const int* __restrict__ qorder,
                                                    int64_t M, const double* __restrict__ state, int k, double r, double r2,
                                                    int* __restrict__ out_idx, double* __restrict__ out_d2,
                                                    int* __restrict__ out_cnt) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t w = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x / kWave);
    if (w >= M) return;  // the whole wave
    const int m = qorder[w];
    double pose[12], q[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = state[kStPose + i];
    moved(pose, src + (int64_t)m * 3, q);
    double box2 = 0.0;  // squared distance of the query to the target's box
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double lo = lv.g[0].lo[a], hi = lv.g[0].hi[a];
        const double out = q[a] < lo ? lo - q[a] : (q[a] > hi ? q[a] - hi : 0.0);
        box2 += out * out;
    }
    box2 = box2 / kReach;
    KList b = {INFINITY, -1, 0, INFINITY, 0x7fffffff};
    double rho = r * kReach;
    bool done = false;
    for (int v = 0; v < lv.count; ++v)
        if (!done)
            done = knn_level(lv.g[v], lv.sp[v], lv.cells[v], q, box2, r2, v + 1 < lv.count ? kLevelShells : 0x7fffffff, k,
                             lane, rho, b);
    if (lane < k) {
        const bool held = lane < b.cnt;
        out_idx[(int64_t)m * k + lane] = held ? b.idx : -1;
        out_d2[(int64_t)m * k + lane] = held ? b.d2 : INFINITY;
    }
    if (lane == 0) out_cnt[m] = b.cnt;
}

// c(q) = #{n : d2 <= r r}, r finite: one query per lane, on the finest level on which the cells that can hold such a point
// span at most kCountSpan + 1 an axis (the last level otherwise).  Every point is in one cell of a level and every cell of the
// cube is visited once; on a hashed level a bucket may hold points of other cells, which are left to their own cell.
__global__ __launch_bounds__(kBlock) void k_icp_radius_count(Levels lv, const double* __restrict__ src,
                                                             const int* __restrict__ qorder, int64_t M,
                                                             const double* __restrict__ state, double r, double r2,
                                                             int* __restrict__ out_cnt) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= M) return;
    const int m = qorder[l];
    double pose[12], q[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[i] = state[kStPose + i];
    moved(pose, src + (int64_t)m * 3, q);
    const double rho = r * kReach;
    int count = 0;
    bool done = false;
    for (int v = 0; v < lv.count; ++v) {
        if (done) continue;
        const CellGrid& g = lv.g[v];
        int lo[3], hi[3], span = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double wide = rho + (fabs(q[a]) + rho) * 0x1p-50;  // the rounding of q_a -+ rho
            lo[a] = min(cell_of(q[a] - wide, g.lo[a], g.edge), g.dim[a] - 1);
            hi[a] = min(cell_of(q[a] + wide, g.lo[a], g.edge), g.dim[a] - 1);
            span = max(span, hi[a] - lo[a]);
        }
        if (span > kCountSpan && v + 1 < lv.count) continue;
        done = true;
        const double4* __restrict__ sp = lv.sp[v];
        const int2* __restrict__ cells = lv.cells[v];
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const int2 be = cells[cell_key(x, y, z, g)];
                    for (int t = be.x; t < be.y; ++t) {
                        const double4 p = sp[t];
                        if (!g.dense && (cell_of(p.x, g.lo[0], g.edge) != x || cell_of(p.y, g.lo[1], g.edge) != y ||
                                         cell_of(p.z, g.lo[2], g.edge) != z))
                            continue;
                        const double dx = p.x - q[0], dy = p.y - q[1], dz = p.z - q[2];
                        count += (dx * dx + dy * dy) + dz * dz <= r2 ? 1 : 0;
                    }
                }
    }
    out_cnt[m] = count;
}

// ------------------------------------------------------------------------------------------------- outlier filters (3.17)
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
        // Open3D's TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0), shift (x3, x4, x5)
        const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
        d[0] = cg * cb; d[1] = cg * sb * sa - sg * ca; d[2] = cg * sb * ca + sg * sa;
        d[3] = sg * cb; d[4] = sg * sb * sa + cg * ca; d[5] = sg * sb * ca - cg * sa;
        d[6] = -sb;     d[7] = cb * sa;                d[8] = cb * ca;
        d[9] = x[3]; d[10] = x[4]; d[11] = x[5];
    }
    double old[12];
    for (int k = 0; k < 12; ++k) old[k] = state[kStPose + k];
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b)
            state[kStPose + 3 * a + b] = (d[3 * a] * old[b] + d[3 * a + 1] * old[3 + b]) + d[3 * a + 2] * old[6 + b];
        state[kStPose + 9 + a] = ((d[3 * a] * old[9] + d[3 * a + 1] * old[10]) + d[3 * a + 2] * old[11]) + d[9 + a];
    }
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

// ------------------------------------------------------------------------------------------------------------ cell edge
// The smallest edge a level may have: below it the cell coordinates of the box would pass kCellMax and pile up in the last
// cell.  With it, kMaxLevels levels of step kLevelStep always reach a level on which the box is at most two cells wide.
double floor_edge(double edge, const double* lo, const double* hi) {
    const double ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    return std::max(edge, std::ldexp(ext, -kFloorBits));
}

// The edge at which the distinct points of a sample of the cloud are at most four to an occupied cell (halving from the
// largest extent, kFloorBits times at the most), carried over to the whole cloud by the dimension the last halving shows:
// occupied cells grow as edge^-D, D in [1, 3].  Copies of a point count once - no edge separates them - so a cloud that
// repeats its points, or whose coordinates are quantised, stops where its distinct points are apart.
double choose_edge(const std::vector<double>& raw, int64_t n, const double* lo, const double* hi) {
    const double ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    if (!(ext > 0.0)) return 1.0;
    const int64_t ns = std::min<int64_t>(n, kSample), stride = n / ns;
    struct P3 {
        double c[3];
        bool operator<(const P3& o) const { return std::lexicographical_compare(c, c + 3, o.c, o.c + 3); }
        bool operator==(const P3& o) const { return c[0] == o.c[0] && c[1] == o.c[1] && c[2] == o.c[2]; }
    };
    std::vector<P3> pts((size_t)ns);
    for (int64_t i = 0; i < ns; ++i)
        for (int a = 0; a < 3; ++a) pts[(size_t)i].c[a] = raw[(size_t)(i * stride) * 3 + a];
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    const double distinct = (double)pts.size();
    std::vector<uint64_t> keys(pts.size());
    double h = ext, before = 1.0, now = 1.0;
    for (int level = 0; level < kFloorBits; ++level) {
        for (size_t i = 0; i < pts.size(); ++i) {
            uint64_t key = 0;
            for (int a = 0; a < 3; ++a) {
                const uint64_t c = (uint64_t)std::floor((pts[i].c[a] - lo[a]) / h);
                key = (key ^ c) * 0x9E3779B97F4A7C15ull;
                key ^= key >> 29;
            }
            keys[i] = key;
        }
        std::sort(keys.begin(), keys.end());
        before = now;
        now = (double)(std::unique(keys.begin(), keys.end()) - keys.begin());
        if (distinct <= 4.0 * now) break;
        h *= 0.5;
    }
    if (n > ns) {
        const double dim = std::min(3.0, std::max(1.0, std::log2(now / before)));
        h *= std::pow((double)ns / (double)n, 1.0 / dim);
    }
    return h;
}

}  // namespace

struct prg_icp {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t N = 0, M = 0;
    bool have_normals = false, have_order = false, have_matches = false;
    int have_knn = 0;                     // k of the lists in knn_*, 0: none
    bool have_counts = false;
    int have_outlier = 0;                 // 0 none, 1 statistical (score, stat, keep), 2 radius (counts, keep)
    bool have_cov[2] = {false, false};    // source, target
    Levels lv;
    prg::DevBuf<double4> tp, tn;          // target points and normals, padded to four doubles
    prg::DevBuf<double4> sp[kMaxLevels];  // per level: the points in cell order, original index in .w
    prg::DevBuf<int2> cells[kMaxLevels];  // per level, table entries: (begin, end)
    prg::DevBuf<double> src;              // [M][3]
    prg::DevBuf<double> cov[2];           // [M][kCov] of the source, [N][kCov] of the target
    prg::DevBuf<unsigned> qkeys;          // 2 M: unsorted, sorted
    prg::DevBuf<int> qvals;               // 2 M: iota, order
    prg::DevBuf<char> sort_tmp;
    prg::DevBuf<int> idx;                 // [M]
    prg::DevBuf<double> d2;               // [M]
    prg::DevBuf<double> part;             // [runs][kSlots]
    prg::DevBuf<double> state;            // [kStLen]
    prg::DevBuf<int> knn_idx;             // [M][k]
    prg::DevBuf<double> knn_d2;           // [M][k]
    prg::DevBuf<int> knn_cnt;             // [M]
    prg::DevBuf<int> counts;              // [M]: the radius count
    prg::DevBuf<double> score;            // [M]: the mean neighbour distance
    prg::DevBuf<double> stat;             // [kOutLen]
    prg::DevBuf<unsigned char> keep;      // [M]
};

namespace {

int require_ready(prg_icp* h, const char* who, bool matches) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "%s: NULL argument", who);
    PRG_REQUIRE(h->N >= 1, PRG_ERR_STATE, "%s: no target (prg_icp_set_target first)", who);
    PRG_REQUIRE(h->M >= 1, PRG_ERR_STATE, "%s: no source (prg_icp_set_source first)", who);
    PRG_REQUIRE(!matches || h->have_matches, PRG_ERR_STATE, "%s: no matches (prg_icp_search first)", who);
    return PRG_OK;
}

// lists, counts and filter results belong to the clouds and the pose they were made with
void drop_lists(prg_icp* h) {
    h->have_knn = 0;
    h->have_counts = false;
    h->have_outlier = 0;
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

// the queries in Morton order of their position under the current pose (once per source / target)
int ensure_order(prg_icp* h) {
    if (h->have_order) return PRG_OK;
    const int64_t M = h->M;
    hipStream_t st = h->stream;
    const CellGrid& g = h->lv.g[0];
    const double ext = std::max(g.hi[0] - g.lo[0], std::max(g.hi[1] - g.lo[1], g.hi[2] - g.lo[2]));
    const double scale = ext > 0.0 ? (double)(1 << kOrderBits) / ext : 0.0;
    size_t need = 0;
    PRG_TRY(prg::sort_pairs_u32(nullptr, &need, h->qkeys.p, h->qkeys.p + M, h->qvals.p, h->qvals.p + M, (unsigned)M,
                                3 * kOrderBits, st));
    PRG_HIP(h->sort_tmp.ensure((int64_t)need + 256, (int64_t)need + 256));
    k_icp_query_keys<<<(unsigned)prg::ceil_div(M, kBlock), kBlock, 0, st>>>(h->src.p, M, h->state.p, g, scale, h->qkeys.p,
                                                                            h->qvals.p);
    PRG_HIP(hipGetLastError());
    PRG_TRY(prg::sort_pairs_u32(h->sort_tmp.p, &need, h->qkeys.p, h->qkeys.p + M, h->qvals.p, h->qvals.p + M, (unsigned)M,
                                3 * kOrderBits, st));
    h->have_order = true;
    return PRG_OK;
}

void enqueue_search(prg_icp* h, double r) {
    k_icp_search<<<(unsigned)prg::ceil_div(h->M, kBlock), kBlock, 0, h->stream>>>(h->lv, h->src.p, h->qvals.p + h->M, h->M,
                                                                                  h->state.p, r, r * r, h->idx.p, h->d2.p);
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

// the k-best lists of every moved source point into knn_*; the buffers grow to M k
int run_knn(prg_icp* h, const char* who, int k, double r) {
    PRG_REQUIRE(k >= 1 && k <= kMaxK, PRG_ERR_INVALID, "%s: k must lie in 1 .. %d, got %d", who, kMaxK, k);
    PRG_REQUIRE(r > 0.0, PRG_ERR_INVALID, "%s: r must be > 0 (infinity: no limit), got %g", who, r);
    const CellGrid& last = h->lv.g[h->lv.count - 1];  // what prg_icp_set_target builds: the kernel deals at most 5^3 cells a shell
    PRG_REQUIRE(std::max(last.dim[0], std::max(last.dim[1], last.dim[2])) <= 2, PRG_ERR_STATE,
                "%s: the last grid level is more than two cells wide", who);
    const int64_t M = h->M;
    h->have_knn = 0;
    if (h->have_outlier == 1) h->have_outlier = 0;  // its keep mask went with these lists
    PRG_HIP(h->knn_idx.ensure(M * k, M * k));
    PRG_HIP(h->knn_d2.ensure(M * k, M * k));
    PRG_HIP(h->knn_cnt.ensure(M, M));
    PRG_TRY(ensure_order(h));
    k_icp_knn<<<(unsigned)prg::ceil_div(M, kBlock / kWave), kBlock, 0, h->stream>>>(
        h->lv, h->src.p, h->qvals.p + M, M, h->state.p, k, r, r * r, h->knn_idx.p, h->knn_d2.p, h->knn_cnt.p);
    PRG_HIP(hipGetLastError());
    h->have_knn = k;
    return PRG_OK;
}

int run_radius_count(prg_icp* h, const char* who, double r) {
    PRG_REQUIRE(r > 0.0 && std::isfinite(r), PRG_ERR_INVALID, "%s: r must be finite and > 0, got %g", who, r);
    const int64_t M = h->M;
    h->have_counts = false;
    if (h->have_outlier == 2) h->have_outlier = 0;  // its keep mask went with these counts
    PRG_HIP(h->counts.ensure(M, M));
    PRG_TRY(ensure_order(h));
    k_icp_radius_count<<<(unsigned)prg::ceil_div(M, kBlock), kBlock, 0, h->stream>>>(h->lv, h->src.p, h->qvals.p + M, M,
                                                                                     h->state.p, r, r * r, h->counts.p);
    PRG_HIP(hipGetLastError());
    h->have_counts = true;
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_icp_create(prg_icp** out, int device, void* hip_stream) {
    PRG_REQUIRE(out != nullptr, PRG_ERR_INVALID, "prg_icp_create: out is NULL");
    int count = 0;
    PRG_HIP(hipGetDeviceCount(&count));
    PRG_REQUIRE(device >= 0 && device < count, PRG_ERR_INVALID, "prg_icp_create: device %d out of range", device);
    prg_icp* h = new (std::nothrow) prg_icp();
    PRG_REQUIRE(h != nullptr, PRG_ERR_NOMEM, "prg_icp_create: out of host memory");
    h->device = device;
    h->stream = (hipStream_t)hip_stream;
    *out = h;
    return PRG_OK;
}

int prg_icp_destroy(prg_icp* h) {
    if (!h) return PRG_OK;
    prg::DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete h;
    return PRG_OK;
}

int prg_icp_set_target(prg_icp* h, const double* points_hd, const double* normals_hd, int64_t n, double cell_edge) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_icp_set_target: NULL argument");
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_icp_set_target: need 1 <= n < 2^31 points, got %lld",
                (long long)n);
    PRG_REQUIRE(cell_edge >= 0.0 && std::isfinite(cell_edge), PRG_ERR_INVALID,
                "prg_icp_set_target: cell_edge must be finite and >= 0 (0: chosen from the cloud), got %g", cell_edge);
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_set_target: hipSetDevice(%d) failed", h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->N = 0;
    h->have_normals = h->have_order = h->have_matches = h->have_cov[1] = false;
    drop_lists(h);
    std::vector<double> raw, pad;
    double lo[3], hi[3];
    PRG_TRY(prg::load_cloud3(points_hd, n, "prg_icp_set_target: the points contain NaN or infinity", raw, pad, lo, hi));
    const double edge0 = floor_edge(cell_edge > 0.0 ? cell_edge : choose_edge(raw, n, lo, hi), lo, hi);
    const unsigned bits = prg::cell_table_bits(n);

    PRG_HIP(h->tp.ensure(n, n));
    PRG_HIP(hipMemcpy(h->tp.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
    if (normals_hd) {
        PRG_TRY(prg::load_cloud3(normals_hd, n, "prg_icp_set_target: the normals contain NaN or infinity", raw, pad, nullptr,
                                 nullptr));
        PRG_HIP(h->tn.ensure(n, n));
        PRG_HIP(hipMemcpy(h->tn.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    prg::CellGridScratch scratch;
    PRG_TRY(scratch.size(n, bits));
    Levels& lv = h->lv;
    lv.count = 0;
    double edge = edge0;
    for (int k = 0; k < kMaxLevels; ++k, edge *= kLevelStep) {  // ends at a level at most two cells wide (floor_edge)
        const CellGrid gr = lv.g[k] = prg::make_cell_grid(lo, hi, edge, bits);
        const int64_t entries = prg::cell_entries(gr);
        PRG_HIP(h->sp[k].ensure(n, n));
        PRG_HIP(h->cells[k].ensure(entries, entries));
        PRG_TRY(prg::build_cell_grid(gr, bits, h->tp.p, n, scratch, h->sp[k].p, h->cells[k].p, st));
        lv.sp[k] = h->sp[k].p;
        lv.cells[k] = h->cells[k].p;
        lv.count = k + 1;
        if (std::max(gr.dim[0], std::max(gr.dim[1], gr.dim[2])) <= 2) break;  // 27 cells hold every point: this level ends any search
    }
    PRG_HIP(hipStreamSynchronize(st));  // the scratch goes away with this scope
    PRG_TRY(ensure_state(h));
    h->N = n;
    h->have_normals = normals_hd != nullptr;
    return PRG_OK;
}

int prg_icp_get_grid(prg_icp* h, double* cell_edge_host, int* dims_host, int* dense_host, int* levels_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_icp_get_grid: NULL argument");
    PRG_REQUIRE(h->N >= 1, PRG_ERR_STATE, "prg_icp_get_grid: no target (prg_icp_set_target first)");
    if (cell_edge_host) *cell_edge_host = h->lv.g[0].edge;
    if (dims_host)
        for (int a = 0; a < 3; ++a) dims_host[a] = h->lv.g[0].dim[a];
    if (dense_host) *dense_host = h->lv.g[0].dense;
    if (levels_host) *levels_host = h->lv.count;
    return PRG_OK;
}

int prg_icp_set_source(prg_icp* h, const double* points_hd, int64_t m) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_icp_set_source: NULL argument");
    PRG_REQUIRE(m >= 1 && m < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_icp_set_source: need 1 <= m < 2^31 points, got %lld",
                (long long)m);
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_set_source: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_set_covariances: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_set_covariances_from_normals: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_covariances: hipSetDevice(%d) failed", h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    const int64_t rows = which == 0 ? h->M : h->N;
    PRG_HIP(hipMemcpy(cov_host, h->cov[which].p, (size_t)rows * kCov * sizeof(double), hipMemcpyDeviceToHost));
    return PRG_OK;
}

int prg_icp_set_pose(prg_icp* h, const double* pose_host) {
    PRG_REQUIRE(h && pose_host, PRG_ERR_INVALID, "prg_icp_set_pose: NULL argument");
    for (int k = 0; k < 12; ++k)
        PRG_REQUIRE(std::isfinite(pose_host[k]), PRG_ERR_INVALID, "prg_icp_set_pose: the pose contains NaN or infinity");
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_set_pose: hipSetDevice(%d) failed", h->device);
    PRG_TRY(ensure_state(h));
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(hipMemcpy(h->state.p + kStPose, pose_host, 12 * sizeof(double), hipMemcpyHostToDevice));
    h->have_matches = false;
    drop_lists(h);
    return PRG_OK;
}

int prg_icp_get_pose(prg_icp* h, double* pose_host) {
    PRG_REQUIRE(h && pose_host, PRG_ERR_INVALID, "prg_icp_get_pose: NULL argument");
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_pose: hipSetDevice(%d) failed", h->device);
    PRG_TRY(ensure_state(h));
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(hipMemcpy(pose_host, h->state.p + kStPose, 12 * sizeof(double), hipMemcpyDeviceToHost));
    return PRG_OK;
}

int prg_icp_search(prg_icp* h, double r) {
    PRG_TRY(require_ready(h, "prg_icp_search", false));
    PRG_REQUIRE(r > 0.0, PRG_ERR_INVALID, "prg_icp_search: r must be > 0 (infinity: no limit), got %g", r);
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_search: hipSetDevice(%d) failed", h->device);
    PRG_TRY(ensure_order(h));
    k_icp_reset<<<1, 1, 0, h->stream>>>(0, h->state.p);
    enqueue_search(h, r);
    PRG_HIP(hipGetLastError());
    h->have_matches = true;
    return PRG_OK;
}

int prg_icp_get_matches(prg_icp* h, int* index_host, double* d2_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_matches", true));
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_matches: hipSetDevice(%d) failed", h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    if (index_host) PRG_HIP(hipMemcpy(index_host, h->idx.p, (size_t)h->M * sizeof(int), hipMemcpyDeviceToHost));
    if (d2_host) PRG_HIP(hipMemcpy(d2_host, h->d2.p, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost));
    return PRG_OK;
}

int prg_icp_sums(prg_icp* h, int kind, double* out_host) {
    PRG_TRY(require_ready(h, "prg_icp_sums", true));
    PRG_REQUIRE(out_host != nullptr, PRG_ERR_INVALID, "prg_icp_sums: NULL argument");
    PRG_TRY(check_kind("prg_icp_sums", h, kind));
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_sums: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_step: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_iterate: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_state: hipSetDevice(%d) failed", h->device);
    PRG_TRY(ensure_state(h));
    double s[kStLen];
    PRG_HIP(hipMemcpyAsync(s, h->state.p, sizeof(s), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    if (pose_host)
        for (int k = 0; k < 12; ++k) pose_host[k] = s[kStPose + k];
    if (count_host) *count_host = (int64_t)s[kStCount];
    if (sum_host) *sum_host = s[kStSum];
    if (n_iter_host) *n_iter_host = (int)s[kStIter];
    if (converged_host) *converged_host = (int)s[kStConverged];
    if (status_host) *status_host = (int)s[kStStatus];
    return PRG_OK;
}

int prg_icp_max_k(int* out) {
    PRG_REQUIRE(out != nullptr, PRG_ERR_INVALID, "prg_icp_max_k: NULL argument");
    *out = kMaxK;
    return PRG_OK;
}

int prg_icp_knn(prg_icp* h, int k, double r) {
    PRG_TRY(require_ready(h, "prg_icp_knn", false));
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_knn: hipSetDevice(%d) failed", h->device);
    return run_knn(h, "prg_icp_knn", k, r);
}

int prg_icp_get_knn(prg_icp* h, int* index_host, double* d2_host, int* count_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_knn", false));
    PRG_REQUIRE(h->have_knn > 0, PRG_ERR_STATE, "prg_icp_get_knn: no lists (prg_icp_knn first)");
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_knn: hipSetDevice(%d) failed", h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    const size_t slots = (size_t)h->M * (size_t)h->have_knn;
    if (index_host) PRG_HIP(hipMemcpy(index_host, h->knn_idx.p, slots * sizeof(int), hipMemcpyDeviceToHost));
    if (d2_host) PRG_HIP(hipMemcpy(d2_host, h->knn_d2.p, slots * sizeof(double), hipMemcpyDeviceToHost));
    if (count_host) PRG_HIP(hipMemcpy(count_host, h->knn_cnt.p, (size_t)h->M * sizeof(int), hipMemcpyDeviceToHost));
    return PRG_OK;
}

int prg_icp_radius_count(prg_icp* h, double r) {
    PRG_TRY(require_ready(h, "prg_icp_radius_count", false));
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_radius_count: hipSetDevice(%d) failed", h->device);
    return run_radius_count(h, "prg_icp_radius_count", r);
}

int prg_icp_get_counts(prg_icp* h, int* count_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_counts", false));
    PRG_REQUIRE(count_host != nullptr, PRG_ERR_INVALID, "prg_icp_get_counts: NULL argument");
    PRG_REQUIRE(h->have_counts, PRG_ERR_STATE, "prg_icp_get_counts: no counts (prg_icp_radius_count first)");
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_counts: hipSetDevice(%d) failed", h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(hipMemcpy(count_host, h->counts.p, (size_t)h->M * sizeof(int), hipMemcpyDeviceToHost));
    return PRG_OK;
}

int prg_icp_outlier_statistical(prg_icp* h, int k, double std_ratio) {
    PRG_TRY(require_ready(h, "prg_icp_outlier_statistical", false));
    PRG_REQUIRE(std_ratio >= 0.0 && std::isfinite(std_ratio), PRG_ERR_INVALID,
                "prg_icp_outlier_statistical: std_ratio must be finite and >= 0, got %g", std_ratio);
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_outlier_statistical: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_outlier_radius: hipSetDevice(%d) failed", h->device);
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
    prg::DeviceGuard g(h->device);
    PRG_REQUIRE(g.ok, PRG_ERR_HIP, "prg_icp_get_outlier: hipSetDevice(%d) failed", h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    if (keep_host) PRG_HIP(hipMemcpy(keep_host, h->keep.p, (size_t)h->M, hipMemcpyDeviceToHost));
    if (score_host) PRG_HIP(hipMemcpy(score_host, h->score.p, (size_t)h->M * sizeof(double), hipMemcpyDeviceToHost));
    if (stat_host) PRG_HIP(hipMemcpy(stat_host, h->stat.p, 3 * sizeof(double), hipMemcpyDeviceToHost));
    return PRG_OK;
}

}  // extern "C"
