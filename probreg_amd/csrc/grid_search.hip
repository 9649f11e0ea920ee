// The cross-cloud search of the ICP plan on the cell grid of cell_grid.h: nearest neighbour, the k
// nearest, and a radius count, of every moved source point among the target.  All in fp64, no floating-point atomics.
//
//   grid     built once per target.  The cell edge comes from the cloud (a few points per occupied cell), never from the
//            search radius.  Coarser levels (edge x kLevelStep each, until the box is one or two cells wide - always reached,
//            see floor_edge) are built the same way: they carry a query that is far from the cloud over the empty space, and
//            the last one bounds every search.
//   search   one query per lane, queries in Morton order of their moved position.  Shells of cells of growing Chebyshev
//            distance s around the query's clamped cell, kLevelShells of them per level and any number on the last level;
//            after shell s of a level with edge h everything unvisited is farther than
//            sqrt((s h)^2 + D^2), D the query's distance to the target's box.  The lane stops when its best d2 is strictly
//            below that bound (shrunk by a hair), when the bound exceeds r, or when every cell that meets the cube of half
//            edge min(r, sqrt(best d2)) around the query is visited (the shells are clipped to that cube).  The result is the
//            minimum of (d2, index) over the visited points, which does not depend on the order of the visits: the grid
//            does not show.
//   knn      the k best instead of the best: one wave per query, the sorted list one entry per lane, in the same walk.
//   count    the points within r, on one level chosen by r.
// The clip, the bound and the shells are those of grid_search.h; walk_level is the one walk over them.
//
// Every decision value is computed with separately rounded multiplications and additions (no contraction into FMAs), so that
// a restatement in plain IEEE arithmetic takes the same branches.
#pragma clang fp contract(off)
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "icp_plan.h"
#include "lattice_sort.h"

using namespace prg::icp;

namespace {

constexpr int kOrderBits = 10;  // per axis, of the Morton key that orders the queries
constexpr int kSample = 16384;  // points that choose the cell edge
constexpr int kWave = 64;
constexpr int kMaxK = kWave;    // one list entry per lane

using prg::CellGrid;
using prg::cell_key;
using prg::kReach;
using prg::Levels;

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
    double q[3];
    moved_query(state, src, m, q);
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

// ----------------------------------------------------------------------------------------------------------------- walk
// What a walk collects is a List: scan() takes in the points of the cells of shell s inside the clip lo .. hi, full() says
// whether a pruning distance exists yet, and worst() is that distance.  The minimum of (d2, index): one lane.
struct Best {
    double d2;
    int idx;

    __device__ __forceinline__ bool full() const { return idx >= 0; }
    __device__ __forceinline__ double worst() const { return d2; }

    // every point of the bucket of cell (cx, cy, cz): d2 = (dx dx + dy dy) + dz dz
    __device__ __forceinline__ void visit(const double4* __restrict__ sp, const int2* __restrict__ cells, const CellGrid& g, int cx,
                                          int cy, int cz, const double (&q)[3]) {
        const int2 be = cells[cell_key(cx, cy, cz, g)];
        for (int t = be.x; t < be.y; ++t) {
            const double4 y = sp[t];
            const double dx = y.x - q[0], dy = y.y - q[1], dz = y.z - q[2];
            const double e2 = (dx * dx + dy * dy) + dz * dz;
            const int i = (int)y.w;
            if (idx < 0 || e2 < d2 || (e2 == d2 && i < idx)) {
                d2 = e2;
                idx = i;
            }
        }
    }

    // row-wise; points beyond r stay in, the kernel drops them at the end
    __device__ __forceinline__ void scan(const CellGrid& g, const double4* __restrict__ sp, const int2* __restrict__ cells,
                                         const double (&q)[3], double, const int (&c)[3], const int (&lo)[3], const int (&hi)[3],
                                         int s) {
        const int z0 = max(c[2] - s, lo[2]), z1 = min(c[2] + s, hi[2]);
        const int y0 = max(c[1] - s, lo[1]), y1 = min(c[1] + s, hi[1]);
        const int xl = c[0] - s, xh = c[0] + s;
        for (int z = z0; z <= z1; ++z) {
            const bool zf = z - c[2] == s || c[2] - z == s;
            for (int y = y0; y <= y1; ++y) {
                if (zf || y - c[1] == s || c[1] - y == s) {  // a face of the shell: the whole row
                    const int x1 = min(xh, hi[0]);
                    for (int x = max(xl, lo[0]); x <= x1; ++x) visit(sp, cells, g, x, y, z, q);
                } else {  // inside: the two ends of the row (s > 0 here)
                    if (xl >= lo[0]) visit(sp, cells, g, xl, y, z, q);
                    if (xh <= hi[0]) visit(sp, cells, g, xh, y, z, q);
                }
            }
        }
    }
};

__device__ __forceinline__ bool key_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

// The k smallest (d2, index) among d2 <= r r, ascending: one wave, entry t of the sorted list in lane t.  `cnt`, `kd2` and
// `kidx` (the last key of a full list: the pruning key) are the same in every lane, and all control flow is wave-uniform.  The
// stop test and the clipping use the k-th d2, and only when the list is full; a shorter list ends by bound > r r or with the
// last cell that matters.
struct KList {
    double d2;
    int idx;
    int cnt;
    double kd2;
    int kidx;
    int k, lane;

    __device__ __forceinline__ bool full() const { return cnt == k; }
    __device__ __forceinline__ double worst() const { return kd2; }

    // One candidate (the same values in every lane) into the list.  A key that is in the list already is a second visit of
    // that point - a coarser level after the hand-over, two cells of one hashed bucket - and is dropped: d2 of a point is the
    // same bits on every visit, and the last key only shrinks, so a point that was once refused or pushed out stays out.
    __device__ __forceinline__ void insert(double cd2, int cidx) {
        const bool mine = lane < cnt;
        const unsigned long long below = __ballot(mine && key_less(d2, idx, cd2, cidx));
        const unsigned long long same = __ballot(mine && d2 == cd2 && idx == cidx);
        const int pos = __popcll(below);  // the list is sorted: `below` is its first pos lanes
        if (same != 0ull || pos >= k) return;
        const double ud2 = __shfl_up(d2, 1);
        const int uidx = __shfl_up(idx, 1);
        if (lane > pos) {
            d2 = ud2;
            idx = uidx;
        } else if (lane == pos) {
            d2 = cd2;
            idx = cidx;
        }
        cnt = min(cnt + 1, k);
    }

    // The clipped cube around shell s is dealt to the lanes, every lane walks the bucket of its cell if that is on the shell,
    // and each round of one point per lane goes into the list in lane order.  lo <= c <= hi: every extent is >= 1, and at
    // most 2 s + 1 <= 5 below the last level (s <= kLevelShells).  The last level is at most two cells wide (run_knn checks
    // what build_levels builds), so a cube has at most 125 cells, 35 of them off the shell, and 32-bit arithmetic deals it.
    __device__ __forceinline__ void scan(const CellGrid& g, const double4* __restrict__ sp, const int2* __restrict__ cells,
                                         const double (&q)[3], double r2, const int (&c)[3], const int (&lo)[3],
                                         const int (&hi)[3], int s) {
        const int x0 = max(c[0] - s, lo[0]), y0 = max(c[1] - s, lo[1]), z0 = max(c[2] - s, lo[2]);
        const int nx = min(c[0] + s, hi[0]) - x0 + 1, ny = min(c[1] + s, hi[1]) - y0 + 1, nz = min(c[2] + s, hi[2]) - z0 + 1;
        const int nxy = nx * ny, total = nxy * nz;
        for (int base = 0; base < total; base += kWave) {
            const int i = base + lane;
            int2 be = make_int2(0, 0);
            if (i < total) {
                const int z = z0 + i / nxy, y = y0 + (i % nxy) / nx, x = x0 + i % nx;
                if (prg::on_shell(x, y, z, c, s)) be = cells[cell_key(x, y, z, g)];
            }
            for (int t = be.x; __ballot(t < be.y) != 0ull; ++t) {
                double e2 = INFINITY;
                int i2 = 0x7fffffff;
                bool cand = false;
                if (t < be.y) {
                    const double4 y = sp[t];
                    const double dx = y.x - q[0], dy = y.y - q[1], dz = y.z - q[2];
                    e2 = (dx * dx + dy * dy) + dz * dz;
                    i2 = (int)y.w;
                    cand = e2 <= r2 && (cnt < k || key_less(e2, i2, kd2, kidx));
                }
                for (unsigned long long todo = __ballot(cand); todo != 0ull; todo &= todo - 1ull) {
                    const int j = __builtin_ctzll(todo);
                    insert(__shfl(e2, j), __shfl(i2, j));
                }
                if (cnt == k) {
                    kd2 = __shfl(d2, k - 1);
                    kidx = __shfl(idx, k - 1);
                }
            }
        }
    }
};

// The shells of one level around the query, clipped to the cells that can hold a point at most rho = min(r, sqrt(worst d2))
// (a hair more) from it.  Returns true when the search is over: the worst d2 of the list is strictly below what anything
// unvisited can have, that bound exceeds r, or every cell that matters has been visited.  false: `shells` shells were not
// enough (never on the last level).
template <class List>
__device__ __forceinline__ bool walk_level(const CellGrid& g, const double4* __restrict__ sp, const int2* __restrict__ cells,
                                           const double (&q)[3], double box2, double r2, int shells, double& rho, List& b) {
    int c[3], lo[3], hi[3];
    prg::centre_cell(q, g, c);
    for (int s = 0;; ++s) {
        prg::clip_cells(q, rho, g, lo, hi);
        if (s > prg::clip_shells(c, lo, hi)) return true;
        if (s > shells) return false;
        b.scan(g, sp, cells, q, r2, c, lo, hi, s);
        const double bound = prg::shell_bound(s, g, box2);
        if ((b.full() && b.worst() < bound) || bound > r2) return true;
        if (b.full()) rho = fmin(rho, sqrt(b.worst()) * kReach);
    }
}

// Source point m under the current pose through the levels, finest first.  The level loop is uniform; a query whose search is
// over sits the coarser levels out.  The list goes in and comes out by value: through a reference both kernels take ten VGPRs
// more, and k_icp_knn loses a wave per SIMD.
template <class List>
__device__ __forceinline__ List walk(const Levels& lv, const double* __restrict__ src, int m, const double* __restrict__ state,
                                     double r, double r2, List b) {
    double q[3];
    moved_query(state, src, m, q);
    const double box2 = prg::box_distance2(q, lv.g[0]);
    double rho = r * kReach;
    bool done = false;
    for (int v = 0; v < lv.count; ++v)
        if (!done)
            done = walk_level(lv.g[v], lv.sp[v], lv.cells[v], q, box2, r2, v + 1 < lv.count ? prg::kLevelShells : 0x7fffffff,
                              rho, b);
    return b;
}

// Lane l serves source point qorder[l] and writes by that index: out_idx (-1: nothing within r) and out_d2 (+inf then).
__global__ __launch_bounds__(kBlock) void k_icp_search(Levels lv, const double* __restrict__ src,
                                                       const int* __restrict__ qorder, int64_t M,
                                                       const double* __restrict__ state, double r, double r2,
                                                       int* __restrict__ out_idx, double* __restrict__ out_d2) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= M || state[kStStop] != 0.0) return;
    const int m = qorder[l];
    const Best b = walk(lv, src, m, state, r, r2, Best{INFINITY, -1});
    const bool hit = b.idx >= 0 && b.d2 <= r2;
    out_idx[m] = hit ? b.idx : -1;
    out_d2[m] = hit ? b.d2 : INFINITY;
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
    const KList b = walk(lv, src, m, state, r, r2, KList{INFINITY, -1, 0, INFINITY, 0x7fffffff, k, lane});
    if (lane < k) {
        const bool held = lane < b.cnt;
        out_idx[(int64_t)m * k + lane] = held ? b.idx : -1;
        out_d2[(int64_t)m * k + lane] = held ? b.d2 : INFINITY;
    }
    if (lane == 0) out_cnt[m] = b.cnt;
}

// d2 = (dx dx + dy dy) + dz dz <= r r: one more
struct CountWithin {
    double q[3];
    double r2;
    int count;

    __device__ __forceinline__ void operator()(const double4& p) {
        const double dx = p.x - q[0], dy = p.y - q[1], dz = p.z - q[2];
        count += (dx * dx + dy * dy) + dz * dz <= r2 ? 1 : 0;
    }
};

// c(q) = #{n : d2 <= r r}, r finite: one query per lane on the radius walk of grid_search.h.
__global__ __launch_bounds__(kBlock) void k_icp_radius_count(Levels lv, const double* __restrict__ src,
                                                             const int* __restrict__ qorder, int64_t M,
                                                             const double* __restrict__ state, double r, double r2,
                                                             int* __restrict__ out_cnt) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= M) return;
    const int m = qorder[l];
    CountWithin c;
    moved_query(state, src, m, c.q);
    c.r2 = r2;
    c.count = 0;
    prg::radius_walk(lv, c.q, r, c);
    out_cnt[m] = c.count;
}

// ------------------------------------------------------------------------------------------------------------ cell edge
// The smallest edge a level may have: below it the cell coordinates of the box would pass kCellMax and pile up in the last
// cell.  With it, kMaxLevels levels of step kLevelStep always reach a level on which the box is at most two cells wide.
double floor_edge(double edge, const double* lo, const double* hi) {
    const double ext = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
    return std::max(edge, std::ldexp(ext, -prg::kFloorBits));
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
    for (int level = 0; level < prg::kFloorBits; ++level) {
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

namespace prg {
namespace icp {

int build_levels(prg_icp* h, const std::vector<double>& raw, int64_t n, const double* lo, const double* hi, double cell_edge) {
    const unsigned bits = cell_table_bits(n);
    CellGridScratch scratch;
    PRG_TRY(scratch.size(n, bits));
    Levels& lv = h->lv;
    lv.count = 0;
    double edge = floor_edge(cell_edge > 0.0 ? cell_edge : choose_edge(raw, n, lo, hi), lo, hi);
    for (int k = 0; k < kMaxLevels; ++k, edge *= kLevelStep) {  // ends at a level at most two cells wide (floor_edge)
        const CellGrid gr = lv.g[k] = make_cell_grid(lo, hi, edge, bits);
        const int64_t entries = cell_entries(gr);
        PRG_HIP(h->sp[k].ensure(n, n));
        PRG_HIP(h->cells[k].ensure(entries, entries));
        PRG_TRY(build_cell_grid(gr, bits, h->tp.p, n, scratch, h->sp[k].p, h->cells[k].p, h->stream));
        lv.sp[k] = h->sp[k].p;
        lv.cells[k] = h->cells[k].p;
        lv.count = k + 1;
        if (std::max(gr.dim[0], std::max(gr.dim[1], gr.dim[2])) <= 2) break;  // 27 cells hold every point: this level ends any search
    }
    PRG_HIP(hipStreamSynchronize(h->stream));  // the scratch goes away with this scope
    return PRG_OK;
}

int ensure_order(prg_icp* h) {
    if (h->have_order) return PRG_OK;
    const int64_t M = h->M;
    hipStream_t st = h->stream;
    const CellGrid& g = h->lv.g[0];
    const double ext = std::max(g.hi[0] - g.lo[0], std::max(g.hi[1] - g.lo[1], g.hi[2] - g.lo[2]));
    const double scale = ext > 0.0 ? (double)(1 << kOrderBits) / ext : 0.0;
    size_t need = 0;
    PRG_TRY(sort_pairs_u32(nullptr, &need, h->qkeys.p, h->qkeys.p + M, h->qvals.p, h->qvals.p + M, (unsigned)M, 3 * kOrderBits,
                           st));
    PRG_HIP(h->sort_tmp.ensure((int64_t)need + 256, (int64_t)need + 256));
    k_icp_query_keys<<<(unsigned)ceil_div(M, kBlock), kBlock, 0, st>>>(h->src.p, M, h->state.p, g, scale, h->qkeys.p, h->qvals.p);
    PRG_HIP(hipGetLastError());
    PRG_TRY(sort_pairs_u32(h->sort_tmp.p, &need, h->qkeys.p, h->qkeys.p + M, h->qvals.p, h->qvals.p + M, (unsigned)M,
                           3 * kOrderBits, st));
    h->have_order = true;
    return PRG_OK;
}

void enqueue_search(prg_icp* h, double r) {
    k_icp_search<<<(unsigned)ceil_div(h->M, kBlock), kBlock, 0, h->stream>>>(h->lv, h->src.p, h->qvals.p + h->M, h->M, h->state.p,
                                                                             r, r * r, h->idx.p, h->d2.p);
}

int run_knn(prg_icp* h, const char* who, int k, double r) {
    PRG_REQUIRE(k >= 1 && k <= kMaxK, PRG_ERR_INVALID, "%s: k must lie in 1 .. %d, got %d", who, kMaxK, k);
    PRG_REQUIRE(r > 0.0, PRG_ERR_INVALID, "%s: r must be > 0 (infinity: no limit), got %g", who, r);
    const CellGrid& last = h->lv.g[h->lv.count - 1];  // what KList::scan relies on
    PRG_REQUIRE(std::max(last.dim[0], std::max(last.dim[1], last.dim[2])) <= 2, PRG_ERR_STATE,
                "%s: the last grid level is more than two cells wide", who);
    const int64_t M = h->M;
    h->have_knn = 0;
    if (h->have_outlier == 1) h->have_outlier = 0;  // its keep mask went with these lists
    PRG_HIP(h->knn_idx.ensure(M * k, M * k));
    PRG_HIP(h->knn_d2.ensure(M * k, M * k));
    PRG_HIP(h->knn_cnt.ensure(M, M));
    PRG_TRY(ensure_order(h));
    k_icp_knn<<<(unsigned)ceil_div(M, kBlock / kWave), kBlock, 0, h->stream>>>(h->lv, h->src.p, h->qvals.p + M, M, h->state.p, k, r,
                                                                               r * r, h->knn_idx.p, h->knn_d2.p, h->knn_cnt.p);
    PRG_HIP(hipGetLastError());
    h->have_knn = k;
    return PRG_OK;
}

int run_radius_count(prg_icp* h, const char* who, double r) {
    PRG_REQUIRE(r > 0.0 && std::isfinite(r), PRG_ERR_INVALID, "%s: r must be finite and > 0, got %g", who, r);
    const int64_t M = h->M;
    h->have_counts = false;
    if (h->have_outlier == 2) h->have_outlier = 0;  // its keep mask went with these counts
    h->have_dbscan = false;                         // and so did the counts of a clustering
    PRG_HIP(h->counts.ensure(M, M));
    PRG_TRY(ensure_order(h));
    k_icp_radius_count<<<(unsigned)ceil_div(M, kBlock), kBlock, 0, h->stream>>>(h->lv, h->src.p, h->qvals.p + M, M, h->state.p, r,
                                                                                r * r, h->counts.p);
    PRG_HIP(hipGetLastError());
    h->have_counts = true;
    return PRG_OK;
}

}  // namespace icp
}  // namespace prg

extern "C" {

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

int prg_icp_get_matches(prg_icp* h, int* index_host, double* d2_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_matches", true));
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(index_host, h->idx, h->M, h->stream));
    PRG_TRY(prg::copy_out(d2_host, h->d2, h->M, h->stream));
    return PRG_OK;
}

int prg_icp_max_k(int* out) {
    PRG_REQUIRE(out != nullptr, PRG_ERR_INVALID, "prg_icp_max_k: NULL argument");
    *out = kMaxK;
    return PRG_OK;
}

int prg_icp_knn(prg_icp* h, int k, double r) {
    PRG_TRY(require_ready(h, "prg_icp_knn", false));
    PRG_ENTER(h->device);
    return run_knn(h, "prg_icp_knn", k, r);
}

int prg_icp_get_knn(prg_icp* h, int* index_host, double* d2_host, int* count_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_knn", false));
    PRG_REQUIRE(h->have_knn > 0, PRG_ERR_STATE, "prg_icp_get_knn: no lists (prg_icp_knn first)");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(index_host, h->knn_idx, h->M * h->have_knn, h->stream));
    PRG_TRY(prg::copy_out(d2_host, h->knn_d2, h->M * h->have_knn, h->stream));
    PRG_TRY(prg::copy_out(count_host, h->knn_cnt, h->M, h->stream));
    return PRG_OK;
}

int prg_icp_radius_count(prg_icp* h, double r) {
    PRG_TRY(require_ready(h, "prg_icp_radius_count", false));
    PRG_ENTER(h->device);
    return run_radius_count(h, "prg_icp_radius_count", r);
}

int prg_icp_get_counts(prg_icp* h, int* count_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_counts", false));
    PRG_REQUIRE(count_host != nullptr, PRG_ERR_INVALID, "prg_icp_get_counts: NULL argument");
    PRG_REQUIRE(h->have_counts, PRG_ERR_STATE, "prg_icp_get_counts: no counts (prg_icp_radius_count first)");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(count_host, h->counts, h->M, h->stream));
    return PRG_OK;
}

}  // extern "C"
