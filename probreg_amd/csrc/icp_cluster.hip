// DBSCAN on the ICP plan: the radius counts of grid_search.hip say which points are core, the radius walk of
// grid_search.h links every core point with its core neighbours in a union-find that never waits (union_find.h) and finds the
// nearest core neighbour of every other point, and a scan of the roots in index order numbers the clusters.  The cloud is both
// target and source at the identity pose.  d2 = (dx dx + dy dy) + dz dz in fp64 without contraction, as the counts; there is no
// floating-point sum and no floating-point atomic here, and every atomic is a 32-bit integer one issued per lane.
#pragma clang fp contract(off)
#include <math.h>

#include <cmath>

#include "block_scan.h"
#include "icp_plan.h"
#include "union_find.h"

using namespace prg::icp;

namespace {

constexpr int kWave = 64;
constexpr int kScanPer = 4;        // indices per lane of the root scan
constexpr int kScanThreads = 1024;  // of the one workgroup that scans the tile counts
constexpr int kTile = kBlock * kScanPer;

// `parent` on the device for union_find.h.  Relaxed, device scope: the union-find needs atomicity and no order, and whatever a
// kernel wrote is visible to the next one on the stream.
struct DeviceParent {
    int* p;
    __device__ __forceinline__ int load(int x) const { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int x, int v) { return atomicMin(p + x, v); }
    __device__ __forceinline__ int compare_swap(int x, int e, int v) { return atomicCAS(p + x, e, v); }
};

// core_i = c_i >= min_points; parent_i = i for a core point, -1 for the others (which never enter the union-find)
__global__ __launch_bounds__(kBlock) void k_dbscan_core(const int* __restrict__ counts, int64_t M, int min_points,
                                                        unsigned char* __restrict__ core, int* __restrict__ parent) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const bool c = counts[i] >= min_points;
    core[i] = c ? 1 : 0;
    parent[i] = c ? (int)i : -1;
}

// What a lane does with a point of the walk: within eps and core, a core lane joins it if its index is the smaller one (the
// pair is met from both ends; the larger end does the work), any other lane keeps the minimum of (d2, index).
struct Link {
    double q[3];
    double r2;
    int self;
    bool is_core;
    const unsigned char* __restrict__ core;
    DeviceParent parent;
    double best_d2;
    int best;

    __device__ __forceinline__ void operator()(const double4& p) {
        const double dx = p.x - q[0], dy = p.y - q[1], dz = p.z - q[2];
        const double e2 = (dx * dx + dy * dy) + dz * dz;
        if (!(e2 <= r2)) return;
        const int j = (int)p.w;
        if (is_core && j >= self) return;
        if (!core[j]) return;
        if (is_core) {
            prg::uf_hook(parent, self, j);  // bounded by self + 1 rounds of at most self steps each (union_find.h)
        } else if (best < 0 || e2 < best_d2 || (e2 == best_d2 && j < best)) {
            best_d2 = e2;
            best = j;
        }
    }
};

// Lane l serves point qorder[l] on the radius walk (every neighbour once, grid_search.h).  near_i: the nearest core neighbour
// of a point that is not core, -1 when it has none or is core itself.
__global__ __launch_bounds__(kBlock) void k_dbscan_link(prg::Levels lv, const double* __restrict__ src,
                                                        const int* __restrict__ qorder, int64_t M,
                                                        const double* __restrict__ state, double r, double r2,
                                                        const unsigned char* __restrict__ core, int* __restrict__ parent,
                                                        int* __restrict__ near) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= M) return;
    const int m = qorder[l];
    Link k;
    moved_query(state, src, m, k.q);
    k.r2 = r2;
    k.self = m;
    k.is_core = core[m] != 0;
    k.core = core;
    k.parent = DeviceParent{parent};
    k.best_d2 = INFINITY;
    k.best = -1;
    prg::radius_walk(lv, k.q, r, k);
    near[m] = k.best;
}

// After the link the roots are final: i is the smallest core index of its cluster iff parent_i == i.
__device__ __forceinline__ int count_roots(const int* __restrict__ parent, int64_t M, int64_t b) {
    int c = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) c += (b + u < M && parent[b + u] == (int)(b + u)) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(kBlock) void k_dbscan_root_count(const int* __restrict__ parent, int64_t M,
                                                              int* __restrict__ tile_count) {
    __shared__ int cnt[kBlock];
    cnt[threadIdx.x] = count_roots(parent, M, ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kScanPer);
    prg::scan_inclusive<kBlock>(cnt);
    if (threadIdx.x == kBlock - 1) tile_count[blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of the tile counts by one workgroup; *total = the number of clusters
__global__ __launch_bounds__(kScanThreads) void k_dbscan_tile_scan(const int* __restrict__ tile_count, int ntiles,
                                                                   int* __restrict__ tile_start, int* __restrict__ total) {
    __shared__ int cnt[kScanThreads];
    prg::tile_scan<kScanThreads>(tile_count, ntiles, tile_start, total, cnt);
}

// id_i = the number of roots below i, for every root i: clusters in ascending order of their smallest core index
__global__ __launch_bounds__(kBlock) void k_dbscan_number(const int* __restrict__ parent, int64_t M,
                                                          const int* __restrict__ tile_start, int* __restrict__ id) {
    __shared__ int cnt[kBlock];
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kScanPer;
    const int c = count_roots(parent, M, b);
    cnt[threadIdx.x] = c;
    prg::scan_inclusive<kBlock>(cnt);
    int pos = tile_start[blockIdx.x] + cnt[threadIdx.x] - c;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int64_t j = b + u;
        if (j < M && parent[j] == (int)j) id[j] = pos++;
    }
}

// label_i = id[root of i] for a core point, id[root of near_i] for a border point, -1 for noise; sizes[label] counts them.
// The roots are final, so find only reads its way up (and shortens it).  The sizes are integer sums, the same whatever the
// order: the lanes of a wave that share a label add their number with one atomic.
__global__ __launch_bounds__(kBlock) void k_dbscan_label(const unsigned char* __restrict__ core, const int* __restrict__ near,
                                                         int* __restrict__ parent, const int* __restrict__ id, int64_t M,
                                                         int* __restrict__ labels, int* __restrict__ sizes) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int label = -1;
    if (i < M) {
        const int from = core[i] ? (int)i : near[i];
        if (from >= 0) {
            DeviceParent par{parent};
            label = id[prg::uf_find(par, from)];  // at most `from` steps (union_find.h)
        }
        labels[i] = label;
    }
    // At most kWave rounds: every round retires the lanes that hold the label of the first lane left, at least that one.
    for (unsigned long long todo = __ballot(label >= 0); todo != 0ull;) {
        const int first = __builtin_ctzll(todo);
        const int which = __shfl(label, first);
        const unsigned long long same = __ballot(label == which) & todo;
        if ((int)(threadIdx.x & (kWave - 1)) == first) atomicAdd(sizes + which, __popcll(same));
        todo &= ~same;
    }
}

}  // namespace

extern "C" {

int prg_icp_dbscan(prg_icp* h, double eps, int min_points) {
    PRG_TRY(require_ready(h, "prg_icp_dbscan", false));
    PRG_REQUIRE(min_points >= 1, PRG_ERR_INVALID, "prg_icp_dbscan: min_points must be >= 1, got %d", min_points);
    PRG_REQUIRE(h->N == h->M, PRG_ERR_STATE,
                "prg_icp_dbscan: the cloud must be set as the target and as the source (%lld and %lld points)", (long long)h->N,
                (long long)h->M);
    PRG_ENTER(h->device);
    PRG_TRY(run_radius_count(h, "prg_icp_dbscan", eps));  // refuses an eps that is not finite and > 0; drops an older clustering
    const int64_t M = h->M;
    const int ntiles = (int)prg::ceil_div(M, kTile);
    PRG_HIP(h->db_core.ensure(M, M));
    PRG_HIP(h->db_parent.ensure(M, M));
    PRG_HIP(h->db_near.ensure(M, M));
    PRG_HIP(h->db_id.ensure(M, M));
    PRG_HIP(h->db_labels.ensure(M, M));
    PRG_HIP(h->db_sizes.ensure(M, M));
    PRG_HIP(h->db_tiles.ensure(2 * (int64_t)ntiles + 1, 2 * (int64_t)ntiles + 1));
    hipStream_t st = h->stream;
    const unsigned blocks = (unsigned)prg::ceil_div(M, kBlock);
    int* const tile_count = h->db_tiles.p;
    int* const tile_start = tile_count + ntiles;
    int* const total = tile_start + ntiles;
    PRG_HIP(hipMemsetAsync(h->db_sizes.p, 0, (size_t)M * sizeof(int), st));
    k_dbscan_core<<<blocks, kBlock, 0, st>>>(h->counts.p, M, min_points, h->db_core.p, h->db_parent.p);
    k_dbscan_link<<<blocks, kBlock, 0, st>>>(h->lv, h->src.p, h->qvals.p + M, M, h->state.p, eps, eps * eps, h->db_core.p,
                                             h->db_parent.p, h->db_near.p);
    k_dbscan_root_count<<<(unsigned)ntiles, kBlock, 0, st>>>(h->db_parent.p, M, tile_count);
    k_dbscan_tile_scan<<<1, kScanThreads, 0, st>>>(tile_count, ntiles, tile_start, total);
    k_dbscan_number<<<(unsigned)ntiles, kBlock, 0, st>>>(h->db_parent.p, M, tile_start, h->db_id.p);
    k_dbscan_label<<<blocks, kBlock, 0, st>>>(h->db_core.p, h->db_near.p, h->db_parent.p, h->db_id.p, M, h->db_labels.p,
                                              h->db_sizes.p);
    PRG_HIP(hipGetLastError());
    h->db_clusters = -1;
    h->have_dbscan = true;
    return PRG_OK;
}

int prg_icp_get_dbscan(prg_icp* h, int* labels_host, unsigned char* core_host, int* n_clusters_host, int* sizes_host) {
    PRG_TRY(require_ready(h, "prg_icp_get_dbscan", false));
    PRG_REQUIRE(h->have_dbscan, PRG_ERR_STATE, "prg_icp_get_dbscan: no clustering (prg_icp_dbscan first)");
    PRG_ENTER(h->device);
    if (h->db_clusters < 0) {
        const int64_t ntiles = prg::ceil_div(h->M, kTile);
        int total = -1;
        PRG_TRY(prg::copy_out(&total, h->db_tiles, 1, h->stream, 2 * ntiles));
        PRG_REQUIRE(total >= 0 && total <= h->M, PRG_ERR_STATE, "prg_icp_get_dbscan: %d clusters of %lld points", total,
                    (long long)h->M);
        h->db_clusters = total;
    }
    if (n_clusters_host) *n_clusters_host = h->db_clusters;
    PRG_TRY(prg::copy_out(labels_host, h->db_labels, h->M, h->stream));
    PRG_TRY(prg::copy_out(core_host, h->db_core, h->M, h->stream));
    PRG_TRY(prg::copy_out(sizes_host, h->db_sizes, h->db_clusters, h->stream));
    return PRG_OK;
}

}  // extern "C"
