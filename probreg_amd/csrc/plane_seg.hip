// Plane segmentation: the RANSAC sweep "hypotheses x points" for the dominant plane of a cloud, all in fp64
// with fixed-order sums and no floating-point atomics.
//
//   prg_plane_build      hypotheses (splitmix64 triples, the degeneracy test, the plane of a triple), one per lane
//   prg_plane_score      the sweep: one valid hypothesis per lane with its plane in registers, the workgroup streams a piece
//                        of kScorePiece points wave-uniformly (scalar loads); the pieces' (count, sum) merged in ascending order
//   prg_plane_best       the winner by (count, sum, h)
//   prg_plane_refine     least-squares refits on the inliers: ten sums in runs of kRefitRun, covariance, smallest eigenvector
//   prg_plane_classify   mask and signed distances of a given plane, its inlier count and ordered sum of dist^2
//   prg_plane_remove     drops the classified inliers: the rest, in ascending index, becomes the handle's cloud
//
// Every decision goes through csrc/plane_seg.h, which the host compiles as well: each of its operations is rounded once, so
// every discrete result (triple, flag, count, winner, mask) and every ordered sum is a function of the input alone.
#include <algorithm>
#include <cmath>
#include <new>

#include "block_scan.h"
#include "dev_buf.h"
#include "plane_seg.h"
#include "prg_common.h"
#include "smallest_eigenvector.h"

namespace {

namespace ps = prg::plane;

constexpr int kBlock = 256;
constexpr int64_t kScoreBatch = 65536;          // hypotheses per scoring launch at most ...
constexpr int64_t kMaxPartials = (int64_t)1 << 24;  // ... and (piece, hypothesis) partials: bound the buffers, not the result
constexpr int64_t kMaxHyp = (int64_t)1 << 24;
constexpr int kBestThreads = 1024;
constexpr int kCompactPer = 16;                      // flags per lane of a compaction
constexpr int kCompactTile = kBlock * kCompactPer;   // flags per workgroup of a compaction
constexpr int kPl = 6;                   // doubles per plane: unit normal, anchor
constexpr int kPt = 4;                   // doubles per packed point (x, y, z, 0) and per packed normal (m_x, m_y, m_z, |m|)
constexpr int kSums = 10;                // the refit's raw sums: k, s (3), sum q q^T (xx, xy, xz, yy, yz, zz)
constexpr int kRefitSlots = 16;

// (x, y, z) rows -> packed points; normals -> (m, |m|) with the length taken here, once
__global__ __launch_bounds__(kBlock) void k_pack(const double* __restrict__ xyz, const double* __restrict__ nxyz, int64_t n,
                                                 double* __restrict__ pts, double* __restrict__ nrm) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    pts[i * kPt + 0] = xyz[i * 3 + 0];
    pts[i * kPt + 1] = xyz[i * 3 + 1];
    pts[i * kPt + 2] = xyz[i * 3 + 2];
    pts[i * kPt + 3] = 0.0;
    if (nxyz) {
        const double mx = nxyz[i * 3 + 0], my = nxyz[i * 3 + 1], mz = nxyz[i * 3 + 2];
        nrm[i * kPt + 0] = mx;
        nrm[i * kPt + 1] = my;
        nrm[i * kPt + 2] = mz;
        nrm[i * kPt + 3] = ps::norm3(mx, my, mz);
    }
}

// ---------------------------------------------------------------------------------------------------------- hypotheses
__global__ __launch_bounds__(kBlock) void k_plane_build(const double* __restrict__ pts, uint32_t n, uint64_t seed,
                                                        uint64_t h_offset, int64_t H, int* __restrict__ tri,
                                                        double* __restrict__ planes, int* __restrict__ valid) {
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    uint32_t id[3];
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        id[j] = ps::draw(seed, h_offset + (uint64_t)h, j, n);  // < n
        tri[h * 3 + j] = (int)id[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[j][a] = pts[(int64_t)id[j] * kPt + a];
    }
    double pl[kPl];
    bool ok = ps::plane_of_triple(p[0], p[1], p[2], pl);
    ok = ok && id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
#pragma unroll
    for (int k = 0; k < kPl; ++k) planes[h * kPl + k] = ok ? pl[k] : 0.0;
    valid[h] = ok ? 1 : 0;
}

// The indices e < n with (flag[e] != 0) == want in ascending order, in three small launches: counts per tile of kCompactTile
// flags, an exclusive scan over the tiles (one workgroup), the order-preserving write.  The scoring sweep takes its valid
// hypotheses from such a list (want = true), prg_plane_remove the points it keeps (want = false: the mask is of the inliers).
__device__ __forceinline__ int count_run(const int* __restrict__ flag, int64_t n, int64_t b, bool want) {
    int c = 0;
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u) c += (b + u < n && (flag[b + u < n ? b + u : 0] != 0) == want) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(kBlock) void k_flag_count(const int* __restrict__ flag, int64_t n, bool want,
                                                       int* __restrict__ tile_count) {
    __shared__ int cnt[kBlock];
    cnt[threadIdx.x] = count_run(flag, n, ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer, want);
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) cnt[threadIdx.x] += cnt[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_count[blockIdx.x] = cnt[0];
}

__global__ __launch_bounds__(kBestThreads) void k_tile_scan(const int* __restrict__ tile_count, int ntiles,
                                                            int* __restrict__ tile_start, int* __restrict__ n_out) {
    __shared__ int cnt[kBestThreads];
    prg::tile_scan<kBestThreads>(tile_count, ntiles, tile_start, n_out, cnt);
}

__global__ __launch_bounds__(kBlock) void k_flag_write(const int* __restrict__ flag, int64_t n, bool want,
                                                       const int* __restrict__ tile_start, int* __restrict__ list) {
    __shared__ int cnt[kBlock];
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer;
    const int c = count_run(flag, n, b, want);
    cnt[threadIdx.x] = c;
    prg::scan_inclusive<kBlock>(cnt);
    int pos = tile_start[blockIdx.x] + cnt[threadIdx.x] - c;  // < the number of listed elements whenever one is written
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u)
        if (b + u < n && (flag[b + u] != 0) == want) list[pos++] = (int)(b + u);
}

// --------------------------------------------------------------------------------------------------------------- score
// what an invalid hypothesis reports: (-1, 0); the valid ones are overwritten by k_score_merge
__global__ __launch_bounds__(kBlock) void k_score_fill(int64_t H, int* __restrict__ counts, double* __restrict__ sums) {
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    counts[h] = -1;
    sums[h] = 0.0;
}

// One valid hypothesis per lane (list[0 .. n_l) of this launch) with its plane in registers; the workgroup streams piece
// blockIdx.x of the points wave-uniformly: the point index is the same in every lane, so the loads are scalar.  Nothing past N
// is read.  part_*: [piece][n_l].
template <bool kNormals>
__global__ __launch_bounds__(kBlock) void k_plane_score(const double* __restrict__ pts, const double* __restrict__ nrm,
                                                        int64_t N, const double* __restrict__ planes,
                                                        const int* __restrict__ list, int64_t n_l, double tau,
                                                        double cos_theta, int* __restrict__ part_count,
                                                        double* __restrict__ part_sum) {
    const int64_t l = (int64_t)blockIdx.y * kBlock + threadIdx.x;
    const int64_t h = list[l < n_l ? l : n_l - 1];  // lanes past the end redo the last hypothesis and store nothing
    double pl[kPl];
#pragma unroll
    for (int k = 0; k < kPl; ++k) pl[k] = planes[h * kPl + k];
    int cnt = 0;
    double sum = 0.0;
    const int64_t c0 = (int64_t)blockIdx.x * ps::kScorePiece;
    const int64_t c1 = c0 + ps::kScorePiece < N ? c0 + ps::kScorePiece : N;
    for (int64_t c = c0; c < c1; ++c) {
        const double* __restrict__ e = pts + c * kPt;
        const double d = ps::distance(pl, e[0], e[1], e[2]);
        bool in = ps::within(d, tau);
        if (kNormals) {
            const double* __restrict__ m = nrm + c * kPt;
            in = in && ps::normal_agrees(pl, m[0], m[1], m[2], m[3], cos_theta);
        }
        cnt += in ? 1 : 0;
        sum = ps::add(sum, in ? ps::mul(d, d) : 0.0);  // + 0.0 is exact: the sum runs over the inliers in ascending index
    }
    if (l < n_l) {
        part_count[(int64_t)blockIdx.x * n_l + l] = cnt;
        part_sum[(int64_t)blockIdx.x * n_l + l] = sum;
    }
}

// piece results in ascending piece order, stored at the hypothesis' own index
__global__ __launch_bounds__(kBlock) void k_score_merge(const int* __restrict__ part_count, const double* __restrict__ part_sum,
                                                        int64_t npiece, const int* __restrict__ list, int64_t n_l,
                                                        int* __restrict__ counts, double* __restrict__ sums) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= n_l) return;
    int cnt = 0;
    double sum = 0.0;
    for (int64_t g = 0; g < npiece; ++g) {
        cnt += part_count[g * n_l + l];
        sum = ps::add(sum, part_sum[g * n_l + l]);
    }
    counts[list[l]] = cnt;
    sums[list[l]] = sum;
}

// one workgroup over the valid hypotheses: best_i = (h or -1, count), best_d = (sum, plane[6])
__global__ __launch_bounds__(kBestThreads) void k_best(const int* __restrict__ counts, const double* __restrict__ sums,
                                                       const double* __restrict__ planes, const int* __restrict__ list,
                                                       int64_t n_valid, int* __restrict__ best_i, double* __restrict__ best_d) {
    __shared__ int sc[kBestThreads], sh[kBestThreads];
    __shared__ double ss[kBestThreads];
    int bc = -1, bh = 0x7fffffff;
    double bs = INFINITY;
    for (int64_t l = threadIdx.x; l < n_valid; l += kBestThreads) {
        const int h = list[l];
        const int c = counts[h];
        const double s = sums[h];
        if (c >= 0 && ps::ranks_ahead(c, s, h, bc, bs, bh)) { bc = c; bs = s; bh = h; }
    }
    sc[threadIdx.x] = bc; ss[threadIdx.x] = bs; sh[threadIdx.x] = bh;
    __syncthreads();
    for (int w = kBestThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int o = threadIdx.x + w;
            if (sc[o] >= 0 && ps::ranks_ahead(sc[o], ss[o], sh[o], sc[threadIdx.x], ss[threadIdx.x], sh[threadIdx.x])) {
                sc[threadIdx.x] = sc[o]; ss[threadIdx.x] = ss[o]; sh[threadIdx.x] = sh[o];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool any = sc[0] >= 0;
        best_i[0] = any ? sh[0] : -1;
        best_i[1] = any ? sc[0] : 0;
        best_d[0] = any ? ss[0] : 0.0;
        for (int k = 0; k < kPl; ++k) best_d[1 + k] = any ? planes[(int64_t)sh[0] * kPl + k] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- refit
template <bool kNormals>
__device__ __forceinline__ bool is_inlier(const double (&pl)[kPl], const double* __restrict__ pts,
                                          const double* __restrict__ nrm, int64_t c, double tau, double cos_theta, double* dist) {
    const double* __restrict__ e = pts + c * kPt;
    const double d = ps::distance(pl, e[0], e[1], e[2]);
    *dist = d;
    bool in = ps::within(d, tau);
    if (kNormals) {
        const double* __restrict__ m = nrm + c * kPt;
        in = in && ps::normal_agrees(pl, m[0], m[1], m[2], m[3], cos_theta);
    }
    return in;
}

// The ten sums over the inliers of the plane in `state`, one run of kRefitRun points per lane in ascending index.
// part: [run][kRefitSlots].
template <bool kNormals>
__global__ __launch_bounds__(kBlock) void k_refit_sums(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t N,
                                                       const double* __restrict__ state, double tau, double cos_theta,
                                                       double* __restrict__ part) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t c0 = r * ps::kRefitRun;
    if (c0 >= N) return;
    const int64_t c1 = c0 + ps::kRefitRun < N ? c0 + ps::kRefitRun : N;
    double pl[kPl], acc[kSums];
#pragma unroll
    for (int k = 0; k < kPl; ++k) pl[k] = state[k];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        double d;
        if (!is_inlier<kNormals>(pl, pts, nrm, c, tau, cos_theta, &d)) continue;
        const double qx = ps::sub(pts[c * kPt + 0], pl[3]), qy = ps::sub(pts[c * kPt + 1], pl[4]),
                     qz = ps::sub(pts[c * kPt + 2], pl[5]);
        acc[0] = ps::add(acc[0], 1.0);
        acc[1] = ps::add(acc[1], qx);
        acc[2] = ps::add(acc[2], qy);
        acc[3] = ps::add(acc[3], qz);
        acc[4] = ps::add(acc[4], ps::mul(qx, qx));
        acc[5] = ps::add(acc[5], ps::mul(qx, qy));
        acc[6] = ps::add(acc[6], ps::mul(qx, qz));
        acc[7] = ps::add(acc[7], ps::mul(qy, qy));
        acc[8] = ps::add(acc[8], ps::mul(qy, qz));
        acc[9] = ps::add(acc[9], ps::mul(qz, qz));
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) part[r * kRefitSlots + k] = acc[k];
}

// One workgroup of kRefitSlots lanes: lane k < kSums adds slot k of the runs in ascending run order; lane 0 then finishes the
// step: the sums go to trace (when given), and with three inliers or more the plane in `state` becomes the least-squares one.
__global__ __launch_bounds__(kRefitSlots) void k_refit_step(const double* __restrict__ part, int64_t nruns,
                                                            double* __restrict__ state, double* __restrict__ trace) {
    __shared__ double tot[kRefitSlots];
    double acc = 0.0;
    if ((int)threadIdx.x < kSums) {
        int64_t r = 0;
        for (; r + 8 <= nruns; r += 8) {  // eight loads in flight; the additions stay in ascending run order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(r + u) * kRefitSlots + threadIdx.x];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = ps::add(acc, v[u]);
        }
        for (; r < nruns; ++r) acc = ps::add(acc, part[r * kRefitSlots + threadIdx.x]);
    }
    tot[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t[kSums];
    for (int k = 0; k < kSums; ++k) {
        t[k] = tot[k];
        if (trace) trace[k] = t[k];
    }
    if (t[0] < 3.0) return;  // the plane is kept
    double c[3], cov[6], n[3];
    ps::covariance(t, c, cov);
    prg::smallest_eigenvector(cov, n);
    ps::fix_sign(n);
    for (int a = 0; a < 3; ++a) {
        state[a] = n[a];
        state[3 + a] = ps::add(state[3 + a], c[a]);
    }
}

// ------------------------------------------------------------------------------------------------------------ classify
template <bool kNormals>
__global__ __launch_bounds__(kBlock) void k_classify(const double* __restrict__ pts, const double* __restrict__ nrm, int64_t N,
                                                     const double* __restrict__ state, double tau, double cos_theta,
                                                     int* __restrict__ mask, double* __restrict__ dist) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= N) return;
    double pl[kPl];
#pragma unroll
    for (int k = 0; k < kPl; ++k) pl[k] = state[k];
    double d;
    mask[c] = is_inlier<kNormals>(pl, pts, nrm, c, tau, cos_theta, &d) ? 1 : 0;
    dist[c] = d;
}

// (count, sum of dist^2) of the inliers of one piece of kScorePiece points per lane, ascending index: the order of the score
__global__ __launch_bounds__(kBlock) void k_piece_sums(const int* __restrict__ mask, const double* __restrict__ dist, int64_t N,
                                                       int* __restrict__ part_count, double* __restrict__ part_sum) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t c0 = g * ps::kScorePiece;
    if (c0 >= N) return;
    const int64_t c1 = c0 + ps::kScorePiece < N ? c0 + ps::kScorePiece : N;
    int cnt = 0;
    double sum = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        const bool in = mask[c] != 0;
        const double d = dist[c];
        cnt += in ? 1 : 0;
        sum = ps::add(sum, in ? ps::mul(d, d) : 0.0);
    }
    part_count[g] = cnt;
    part_sum[g] = sum;
}

// the pieces in ascending order, by one lane: out_i = count, out_d = sum
__global__ void k_piece_total(const int* __restrict__ part_count, const double* __restrict__ part_sum, int64_t npiece,
                              int* __restrict__ out_i, double* __restrict__ out_d) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int cnt = 0;
    double sum = 0.0;
    for (int64_t g = 0; g < npiece; ++g) {
        cnt += part_count[g];
        sum = ps::add(sum, part_sum[g]);
    }
    out_i[0] = cnt;
    out_d[0] = sum;
}

// packed rows list[0 .. n_keep) of the old cloud become rows 0 .. n_keep - 1 of the new one
__global__ __launch_bounds__(kBlock) void k_gather(const double* __restrict__ pts, const double* __restrict__ nrm,
                                                   const int* __restrict__ list, int64_t n_keep, double* __restrict__ pts_out,
                                                   double* __restrict__ nrm_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_keep * kPt) return;
    const int64_t i = e / kPt;
    const int k = (int)(e - i * kPt);
    const int64_t src = list[i];
    pts_out[e] = pts[src * kPt + k];
    if (nrm) nrm_out[e] = nrm[src * kPt + k];
}

bool finite6(const double* p) {
    for (int k = 0; k < kPl; ++k)
        if (!std::isfinite(p[k])) return false;
    return true;
}

}  // namespace

struct prg_plane {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t N = 0, H = 0;            // points of the current cloud (prg_plane_remove lowers it), hypotheses
    bool have_normals = false, have_triples = false, have_scores = false, have_mask = false;
    prg::DevBuf<double> pts, nrm, pts_alt, nrm_alt;  // [N][kPt]; the _alt pair receives the compacted cloud and is swapped in
    prg::DevBuf<double> planes;      // [H][kPl]
    prg::DevBuf<int> valid, tri;     // [H], [H][3]
    prg::DevBuf<int> counts, part_count;
    prg::DevBuf<double> sums, part_sum;
    prg::DevBuf<double> refit_part, state, trace, best_d, dist, total_d;
    prg::DevBuf<int> mask, best_i, total_i, piece_count;
    prg::DevBuf<double> piece_sum;
    prg::DevBuf<int> tile_count, tile_start;
    prg::DevBuf<int> list, n_list_dev;   // the valid hypotheses in ascending order, and how many
    prg::DevBuf<int> keep;               // the points prg_plane_remove keeps
    int64_t n_valid = 0;
};

namespace {

// `list` <- the ascending indices e < n with (flag[e] != 0) == want; *n_out: how many.  Drains the stream.
int compact(prg_plane* h, const int* flag, int64_t n, bool want, prg::DevBuf<int>& list, int* n_out) {
    hipStream_t st = h->stream;
    const int ntiles = (int)prg::ceil_div(n, kCompactTile);
    PRG_HIP(h->tile_count.ensure(ntiles, ntiles));
    PRG_HIP(h->tile_start.ensure(ntiles, ntiles));
    PRG_HIP(h->n_list_dev.ensure(1, 1));
    PRG_HIP(list.ensure(n, n));
    k_flag_count<<<ntiles, kBlock, 0, st>>>(flag, n, want, h->tile_count.p);
    k_tile_scan<<<1, kBestThreads, 0, st>>>(h->tile_count.p, ntiles, h->tile_start.p, h->n_list_dev.p);
    k_flag_write<<<ntiles, kBlock, 0, st>>>(flag, n, want, h->tile_start.p, list.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(n_out, h->n_list_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

int ensure_hypotheses(prg_plane* h, int64_t H) {
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->H = 0;
    h->have_triples = h->have_scores = false;
    PRG_HIP(h->planes.ensure(H * kPl, H * kPl));
    PRG_HIP(h->valid.ensure(H, H));
    PRG_HIP(h->tri.ensure(H * 3, H * 3));
    PRG_HIP(h->counts.ensure(H, H));
    PRG_HIP(h->sums.ensure(H, H));
    return PRG_OK;
}

int check_threshold(const char* who, const prg_plane* h, double tau, double cos_theta) {
    PRG_REQUIRE(std::isfinite(tau) && tau >= 0.0, PRG_ERR_INVALID, "%s: tau must be finite and >= 0, got %g", who, tau);
    PRG_REQUIRE(cos_theta < 0.0 || cos_theta <= 1.0, PRG_ERR_INVALID,
                "%s: cos_theta must lie in [0, 1], or be negative for no normal test; got %g", who, cos_theta);
    PRG_REQUIRE(h->N >= 1, PRG_ERR_STATE, "%s: no points (prg_plane_set_points first)", who);
    PRG_REQUIRE(cos_theta < 0.0 || h->have_normals, PRG_ERR_STATE, "%s: a normal test needs normals (prg_plane_set_points)", who);
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_plane_create(prg_plane** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_plane_destroy(prg_plane* h) {
    return prg::destroy_handle(h);
}

int prg_plane_set_points(prg_plane* h, const double* points_hd, const double* normals_hd, int64_t n) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_plane_set_points: NULL argument");
    PRG_REQUIRE(n >= 3 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_plane_set_points: need 3 <= n < 2^31 points, got %lld",
                (long long)n);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->N = 0;
    h->have_normals = h->have_scores = h->have_mask = false;
    prg::DevBuf<double> raw, raw_n;
    PRG_HIP(raw.reset(n * 3));
    if (normals_hd) PRG_HIP(raw_n.reset(n * 3));
    PRG_HIP(h->pts.ensure(n * kPt, n * kPt));
    if (normals_hd) PRG_HIP(h->nrm.ensure(n * kPt, n * kPt));
    PRG_HIP(h->mask.ensure(n, n));
    PRG_HIP(h->dist.ensure(n, n));
    const int64_t nruns = prg::ceil_div(n, ps::kRefitRun), npiece = prg::ceil_div(n, ps::kScorePiece);
    PRG_HIP(h->refit_part.ensure(nruns * kRefitSlots, nruns * kRefitSlots));
    PRG_HIP(h->piece_count.ensure(npiece, npiece));
    PRG_HIP(h->piece_sum.ensure(npiece, npiece));
    PRG_HIP(h->state.ensure(kPl, kPl));
    PRG_HIP(h->total_i.ensure(1, 1));
    PRG_HIP(h->total_d.ensure(1, 1));
    PRG_HIP(hipMemcpyAsync(raw.p, points_hd, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, st));
    if (normals_hd) PRG_HIP(hipMemcpyAsync(raw_n.p, normals_hd, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, st));
    k_pack<<<(unsigned)prg::ceil_div(n, kBlock), kBlock, 0, st>>>(raw.p, raw_n.p, n, h->pts.p, h->nrm.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(st));
    h->N = n;
    h->have_normals = normals_hd != nullptr;
    return PRG_OK;
}

int prg_plane_count(prg_plane* h, int64_t* n_host) {
    PRG_REQUIRE(h && n_host, PRG_ERR_INVALID, "prg_plane_count: NULL argument");
    *n_host = h->N;
    return PRG_OK;
}

int prg_plane_build(prg_plane* h, uint64_t seed, uint64_t h_offset, int64_t H) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_plane_build: NULL argument");
    PRG_REQUIRE(H >= 1 && H <= kMaxHyp, PRG_ERR_INVALID, "prg_plane_build: need 1 <= H <= %lld hypotheses, got %lld",
                (long long)kMaxHyp, (long long)H);
    PRG_REQUIRE(h->N >= 1, PRG_ERR_STATE, "prg_plane_build: no points (prg_plane_set_points first)");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_hypotheses(h, H));
    k_plane_build<<<(unsigned)prg::ceil_div(H, kBlock), kBlock, 0, h->stream>>>(h->pts.p, (uint32_t)h->N, seed, h_offset, H,
                                                                               h->tri.p, h->planes.p, h->valid.p);
    PRG_HIP(hipGetLastError());
    h->H = H;
    h->have_triples = true;
    return PRG_OK;
}

int prg_plane_get_hypotheses(prg_plane* h, int* triples_host, double* planes_host, int* valid_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_plane_get_hypotheses: NULL argument");
    PRG_REQUIRE(h->H >= 1, PRG_ERR_STATE, "prg_plane_get_hypotheses: prg_plane_build or prg_plane_set_hypotheses first");
    PRG_REQUIRE(!triples_host || h->have_triples, PRG_ERR_STATE,
                "prg_plane_get_hypotheses: hypotheses installed by prg_plane_set_hypotheses carry no triples");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(triples_host, h->tri, h->H * 3, h->stream));
    PRG_TRY(prg::copy_out(planes_host, h->planes, h->H * kPl, h->stream));
    PRG_TRY(prg::copy_out(valid_host, h->valid, h->H, h->stream));
    return PRG_OK;
}

int prg_plane_set_hypotheses(prg_plane* h, const double* planes_hd, const int* valid_hd, int64_t H) {
    PRG_REQUIRE(h && planes_hd && valid_hd, PRG_ERR_INVALID, "prg_plane_set_hypotheses: NULL argument");
    PRG_REQUIRE(H >= 1 && H <= kMaxHyp, PRG_ERR_INVALID, "prg_plane_set_hypotheses: need 1 <= H <= %lld hypotheses, got %lld",
                (long long)kMaxHyp, (long long)H);
    PRG_ENTER(h->device);
    PRG_TRY(ensure_hypotheses(h, H));
    PRG_TRY(prg::copy_in(h->planes, planes_hd, H * kPl, h->stream));
    PRG_TRY(prg::copy_in(h->valid, valid_hd, H, h->stream));
    h->H = H;
    return PRG_OK;
}

int prg_plane_score(prg_plane* h, double tau, double cos_theta) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_plane_score: NULL argument");
    PRG_TRY(check_threshold("prg_plane_score", h, tau, cos_theta));
    PRG_REQUIRE(h->H >= 1, PRG_ERR_STATE, "prg_plane_score: no hypotheses (prg_plane_build or prg_plane_set_hypotheses first)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    h->have_scores = false;
    int n_valid = 0;
    PRG_TRY(compact(h, h->valid.p, h->H, true, h->list, &n_valid));
    h->n_valid = n_valid;
    k_score_fill<<<(unsigned)prg::ceil_div(h->H, kBlock), kBlock, 0, st>>>(h->H, h->counts.p, h->sums.p);
    const int64_t npiece = prg::ceil_div(h->N, ps::kScorePiece);
    // hypotheses per launch: a multiple of the workgroup, within the two bounds, never more than there are
    int64_t batch = std::min<int64_t>(kScoreBatch, std::max<int64_t>(kBlock, kMaxPartials / npiece / kBlock * kBlock));
    batch = std::max<int64_t>(1, std::min<int64_t>(batch, h->n_valid));
    PRG_HIP(h->part_count.ensure(npiece * batch, npiece * batch));
    PRG_HIP(h->part_sum.ensure(npiece * batch, npiece * batch));
    const bool normals = cos_theta >= 0.0;
    for (int64_t l0 = 0; l0 < h->n_valid; l0 += batch) {
        const int64_t n_l = std::min<int64_t>(batch, h->n_valid - l0);
        const dim3 grid((unsigned)npiece, (unsigned)prg::ceil_div(n_l, kBlock));
        if (normals)
            k_plane_score<true><<<grid, kBlock, 0, st>>>(h->pts.p, h->nrm.p, h->N, h->planes.p, h->list.p + l0, n_l, tau,
                                                         cos_theta, h->part_count.p, h->part_sum.p);
        else
            k_plane_score<false><<<grid, kBlock, 0, st>>>(h->pts.p, nullptr, h->N, h->planes.p, h->list.p + l0, n_l, tau,
                                                          cos_theta, h->part_count.p, h->part_sum.p);
        k_score_merge<<<grid.y, kBlock, 0, st>>>(h->part_count.p, h->part_sum.p, npiece, h->list.p + l0, n_l, h->counts.p,
                                                 h->sums.p);
    }
    PRG_HIP(hipGetLastError());
    h->have_scores = true;
    return PRG_OK;
}

int prg_plane_get_scores(prg_plane* h, int* counts_host, double* sums_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_plane_get_scores: NULL argument");
    PRG_REQUIRE(h->have_scores, PRG_ERR_STATE, "prg_plane_get_scores: prg_plane_score first");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(counts_host, h->counts, h->H, h->stream));
    PRG_TRY(prg::copy_out(sums_host, h->sums, h->H, h->stream));
    return PRG_OK;
}

int prg_plane_best(prg_plane* h, int64_t* index_host, int64_t* n_valid_host, int* count_host, double* sum_host,
                   double* plane_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_plane_best: NULL argument");
    PRG_REQUIRE(h->have_scores, PRG_ERR_STATE, "prg_plane_best: prg_plane_score first");
    PRG_ENTER(h->device);
    PRG_HIP(h->best_i.ensure(2, 2));
    PRG_HIP(h->best_d.ensure(1 + kPl, 1 + kPl));
    k_best<<<1, kBestThreads, 0, h->stream>>>(h->counts.p, h->sums.p, h->planes.p, h->list.p, h->n_valid, h->best_i.p,
                                              h->best_d.p);
    PRG_HIP(hipGetLastError());
    int bi[2];
    double bd[1 + kPl];
    PRG_HIP(hipMemcpyAsync(bi, h->best_i.p, sizeof(bi), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipMemcpyAsync(bd, h->best_d.p, sizeof(bd), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    if (index_host) *index_host = bi[0];  // -1: no hypothesis is valid
    if (n_valid_host) *n_valid_host = h->n_valid;
    if (count_host) *count_host = bi[1];
    if (sum_host) *sum_host = bd[0];
    if (plane_host)
        for (int k = 0; k < kPl; ++k) plane_host[k] = bd[1 + k];
    return PRG_OK;
}

int prg_plane_refine(prg_plane* h, double tau, double cos_theta, int iters, double* plane_io_host, double* trace_host) {
    PRG_REQUIRE(h && plane_io_host, PRG_ERR_INVALID, "prg_plane_refine: NULL argument");
    PRG_TRY(check_threshold("prg_plane_refine", h, tau, cos_theta));
    PRG_REQUIRE(iters >= 0 && iters <= 1000, PRG_ERR_INVALID, "prg_plane_refine: iters must lie in 0 .. 1000, got %d", iters);
    PRG_REQUIRE(finite6(plane_io_host), PRG_ERR_INVALID, "prg_plane_refine: the plane contains NaN or infinity");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    PRG_HIP(h->trace.ensure((int64_t)std::max(iters, 1) * kSums, (int64_t)std::max(iters, 1) * kSums));
    PRG_HIP(hipMemcpyAsync(h->state.p, plane_io_host, kPl * sizeof(double), hipMemcpyHostToDevice, st));
    const int64_t nruns = prg::ceil_div(h->N, ps::kRefitRun);
    const unsigned nb = (unsigned)prg::ceil_div(nruns, kBlock);
    for (int it = 0; it < iters; ++it) {
        if (cos_theta >= 0.0)
            k_refit_sums<true><<<nb, kBlock, 0, st>>>(h->pts.p, h->nrm.p, h->N, h->state.p, tau, cos_theta, h->refit_part.p);
        else
            k_refit_sums<false><<<nb, kBlock, 0, st>>>(h->pts.p, nullptr, h->N, h->state.p, tau, cos_theta, h->refit_part.p);
        k_refit_step<<<1, kRefitSlots, 0, st>>>(h->refit_part.p, nruns, h->state.p, h->trace.p + (int64_t)it * kSums);
    }
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(plane_io_host, h->state.p, kPl * sizeof(double), hipMemcpyDeviceToHost, st));
    if (trace_host && iters > 0)
        PRG_HIP(hipMemcpyAsync(trace_host, h->trace.p, (size_t)iters * kSums * sizeof(double), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

int prg_plane_classify(prg_plane* h, const double* plane_host, double tau, double cos_theta, int* mask_host, double* dist_host,
                       int* count_host, double* sum_host) {
    PRG_REQUIRE(h && plane_host, PRG_ERR_INVALID, "prg_plane_classify: NULL argument");
    PRG_TRY(check_threshold("prg_plane_classify", h, tau, cos_theta));
    PRG_REQUIRE(finite6(plane_host), PRG_ERR_INVALID, "prg_plane_classify: the plane contains NaN or infinity");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    h->have_mask = false;
    PRG_HIP(hipStreamSynchronize(st));
    PRG_HIP(hipMemcpyAsync(h->state.p, plane_host, kPl * sizeof(double), hipMemcpyHostToDevice, st));
    const unsigned nb = (unsigned)prg::ceil_div(h->N, kBlock);
    if (cos_theta >= 0.0)
        k_classify<true><<<nb, kBlock, 0, st>>>(h->pts.p, h->nrm.p, h->N, h->state.p, tau, cos_theta, h->mask.p, h->dist.p);
    else
        k_classify<false><<<nb, kBlock, 0, st>>>(h->pts.p, nullptr, h->N, h->state.p, tau, cos_theta, h->mask.p, h->dist.p);
    const int64_t npiece = prg::ceil_div(h->N, ps::kScorePiece);
    k_piece_sums<<<(unsigned)prg::ceil_div(npiece, kBlock), kBlock, 0, st>>>(h->mask.p, h->dist.p, h->N, h->piece_count.p,
                                                                            h->piece_sum.p);
    k_piece_total<<<1, 1, 0, st>>>(h->piece_count.p, h->piece_sum.p, npiece, h->total_i.p, h->total_d.p);
    PRG_HIP(hipGetLastError());
    h->have_mask = true;
    PRG_TRY(prg::copy_out(mask_host, h->mask, h->N, st));
    PRG_TRY(prg::copy_out(dist_host, h->dist, h->N, st));
    PRG_TRY(prg::copy_out(count_host, h->total_i, 1, st));
    PRG_TRY(prg::copy_out(sum_host, h->total_d, 1, st));
    return PRG_OK;
}

int prg_plane_remove(prg_plane* h, int64_t* n_left_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_plane_remove: NULL argument");
    PRG_REQUIRE(h->have_mask, PRG_ERR_STATE, "prg_plane_remove: prg_plane_classify first");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    int n_keep = 0;
    PRG_TRY(compact(h, h->mask.p, h->N, false, h->keep, &n_keep));
    h->have_mask = h->have_scores = false;
    h->H = 0;  // the hypotheses were drawn from the old cloud
    if (n_keep > 0) {
        PRG_HIP(h->pts_alt.ensure((int64_t)n_keep * kPt, h->N * kPt));
        if (h->have_normals) PRG_HIP(h->nrm_alt.ensure((int64_t)n_keep * kPt, h->N * kPt));
        k_gather<<<(unsigned)prg::ceil_div((int64_t)n_keep * kPt, kBlock), kBlock, 0, st>>>(
            h->pts.p, h->have_normals ? h->nrm.p : nullptr, h->keep.p, n_keep, h->pts_alt.p, h->nrm_alt.p);
        PRG_HIP(hipGetLastError());
        PRG_HIP(hipStreamSynchronize(st));
        h->pts.swap(h->pts_alt);
        if (h->have_normals) h->nrm.swap(h->nrm_alt);
    }
    h->N = n_keep;
    if (n_left_host) *n_left_host = n_keep;
    return PRG_OK;
}

}  // extern "C"
