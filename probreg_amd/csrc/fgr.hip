// Fast global registration (Zhou, Park, Koltun, ECCV 2016): one pose for all correspondences by Gauss-Newton
// under a Geman-McClure line process whose scale mu is annealed, after a tuple test that removes most wrong matches.  All in
// fp64 with fixed-order sums and no floating-point atomics; every number is defined by csrc/fgr.h.
//
//   prg_fgr_normalise   means of both clouds (runs of 64 rows, ascending), the largest distance from a mean, the matched
//                       pairs in normalised coordinates
//   prg_fgr_tuples      trials in chunks, one per lane: the draw, the three edge tests; the passing trials of a chunk in
//                       ascending order (ordered compaction), the first `maximum_tuple_count` of them accepted
//   prg_fgr_set_used    the pairs the optimisation runs on, gathered into one array
//   prg_fgr_sums        one run of 64 pairs per lane at the state's pose and mu, then the runs added in ascending order
//   prg_fgr_step        one lane: the Cholesky solve, the pose update (pose_step.h, shared with icp.hip), the mu schedule
//   prg_fgr_iterate     "sums, step" n times; pose, mu, status and counters stay on the device
#pragma clang fp contract(off)
#include <algorithm>
#include <cmath>
#include <new>

#include "block_scan.h"
#include "dev_buf.h"
#include "fgr.h"
#include "pose_step.h"
#include "prg_common.h"

namespace {

namespace fg = prg::fgr;

constexpr int kBlock = 256;
constexpr int kScanThreads = 1024;
constexpr int kCompactPer = 16;                      // flags per lane of the compaction
constexpr int kCompactTile = kBlock * kCompactPer;   // flags per workgroup of the compaction
constexpr int64_t kDefaultChunk = 65536;             // trials per launch: bounds the flag buffers, not the result
constexpr int64_t kMaxChunk = (int64_t)1 << 22;
constexpr int64_t kMaxTuples = (int64_t)1 << 24;
constexpr int kPq = 6;           // doubles per pair: p, q
constexpr int kSlots = 32;       // doubles per run of the sums (fg::kSums used)
constexpr int kMeanSlots = 4;
constexpr int kIterChunk = 32;   // iterations enqueued between two looks at the stop flag
constexpr int kStatusOk = 0, kStatusTooFew = 1, kStatusDegenerate = 2;
// norm (doubles): mean_p, mean_q, scale, scale_global
constexpr int kNmMeanP = 0, kNmMeanQ = 3, kNmScale = 6, kNmScaleGlobal = 7, kNmLen = 8;
// state (doubles): the pose, mu, the stop flag, the status, the steps done, the 28 sums
constexpr int kStPose = 0, kStMu = 12, kStStop = 13, kStStatus = 14, kStIter = 15, kStSums = 16, kStLen = 48;

// ----------------------------------------------------------------------------------------------------------- normalise
// One run of kRun rows per lane, ascending: part[run][kMeanSlots] = the sums of x, y, z.
__global__ __launch_bounds__(kBlock) void k_fgr_run_sums(const double* __restrict__ pts, int64_t n, double* __restrict__ part) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i0 = r * fg::kRun;
    if (i0 >= n) return;
    const int64_t i1 = i0 + fg::kRun < n ? i0 + fg::kRun : n;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = i0; i < i1; ++i)
#pragma unroll
        for (int a = 0; a < 3; ++a) acc[a] = fg::add(acc[a], pts[i * 3 + a]);
#pragma unroll
    for (int a = 0; a < 3; ++a) part[r * kMeanSlots + a] = acc[a];
}

// lane a < 3 adds component a of the runs in ascending order and divides by the count
__global__ __launch_bounds__(kMeanSlots) void k_fgr_mean(const double* __restrict__ part, int64_t nruns, int64_t n,
                                                         double* __restrict__ mean) {
    if (threadIdx.x >= 3) return;
    double acc = 0.0;
    int64_t r = 0;
    for (; r + 16 <= nruns; r += 16) {  // sixteen loads in flight; the additions stay in ascending run order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = part[(r + u) * kMeanSlots + threadIdx.x];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = fg::add(acc, v[u]);
    }
    for (; r < nruns; ++r) acc = fg::add(acc, part[r * kMeanSlots + threadIdx.x]);
    mean[threadIdx.x] = fg::quot(acc, (double)n);
}

// the largest |x - mean|^2 of a workgroup's rows (a maximum does not depend on its order)
__global__ __launch_bounds__(kBlock) void k_fgr_far(const double* __restrict__ pts, int64_t n, const double* __restrict__ mean,
                                                    double* __restrict__ part) {
    __shared__ double far[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double d2 = 0.0;
    if (i < n) {
        const double dx = fg::sub(pts[i * 3], mean[0]), dy = fg::sub(pts[i * 3 + 1], mean[1]), dz = fg::sub(pts[i * 3 + 2], mean[2]);
        d2 = fg::add(fg::add(fg::mul(dx, dx), fg::mul(dy, dy)), fg::mul(dz, dz));
    }
    far[threadIdx.x] = d2;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) far[threadIdx.x] = fmax(far[threadIdx.x], far[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = far[0];
}

// scale = the root of the largest squared distance of both clouds (the root is monotone and rounded once)
__global__ __launch_bounds__(kBlock) void k_fgr_scale(const double* __restrict__ part, int64_t nparts, int use_absolute_scale,
                                                      double* __restrict__ norm) {
    __shared__ double far[kBlock];
    double m = 0.0;
    for (int64_t b = threadIdx.x; b < nparts; b += kBlock) m = fmax(m, part[b]);
    far[threadIdx.x] = m;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) far[threadIdx.x] = fmax(far[threadIdx.x], far[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double scale = fg::root(far[0]);
        norm[kNmScale] = scale;
        norm[kNmScaleGlobal] = use_absolute_scale ? 1.0 : scale;
    }
}

// pair c in normalised coordinates; an index outside its cloud raises `bad` and reads nothing
__global__ __launch_bounds__(kBlock) void k_fgr_pack(const double* __restrict__ src, int64_t M, const double* __restrict__ tgt,
                                                     int64_t N, const int* __restrict__ corr, int64_t C,
                                                     const double* __restrict__ norm, double* __restrict__ pq,
                                                     int* __restrict__ bad) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    const int64_t i = corr[c * 2], j = corr[c * 2 + 1];
    const bool ok = i >= 0 && i < M && j >= 0 && j < N;
    if (!ok) bad[0] = 1;
    const double sg = norm[kNmScaleGlobal];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pq[c * kPq + a] = ok ? fg::normalised(src[i * 3 + a], norm[kNmMeanP + a], sg) : 0.0;
        pq[c * kPq + 3 + a] = ok ? fg::normalised(tgt[j * 3 + a], norm[kNmMeanQ + a], sg) : 0.0;
    }
}

// -------------------------------------------------------------------------------------------------------------- tuples
// trial t0 + e per lane, e < n: flag[e] = the tuple test of its three pairs
__global__ __launch_bounds__(kBlock) void k_fgr_trials(const double* __restrict__ pq, uint32_t C, uint64_t seed, uint64_t t0,
                                                       int64_t n, double s, int* __restrict__ flag) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n) return;
    double p[3][3], q[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int64_t id = fg::draw(seed, t0 + (uint64_t)e, j, C);  // < C
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[j][a] = pq[id * kPq + a];
            q[j][a] = pq[id * kPq + 3 + a];
        }
    }
    flag[e] = fg::tuple_passes(p, q, s) ? 1 : 0;
}

// The set flags of a chunk in ascending order, as global_reg.hip lists its valid hypotheses: counts per tile of kCompactTile
// flags, an exclusive scan over the tiles (one workgroup), the order-preserving write.
__device__ __forceinline__ int count_run(const int* __restrict__ flag, int64_t n, int64_t b) {
    int c = 0;
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u) c += (b + u < n && flag[b + u < n ? b + u : 0] != 0) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(kBlock) void k_fgr_flag_count(const int* __restrict__ flag, int64_t n, int* __restrict__ tile_count) {
    __shared__ int cnt[kBlock];
    cnt[threadIdx.x] = count_run(flag, n, ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer);
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) cnt[threadIdx.x] += cnt[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_count[blockIdx.x] = cnt[0];
}

__global__ __launch_bounds__(kScanThreads) void k_fgr_tile_scan(const int* __restrict__ tile_count, int ntiles,
                                                                int* __restrict__ tile_start, int* __restrict__ n_out) {
    __shared__ int cnt[kScanThreads];
    prg::tile_scan<kScanThreads>(tile_count, ntiles, tile_start, n_out, cnt);
}

__global__ __launch_bounds__(kBlock) void k_fgr_flag_write(const int* __restrict__ flag, int64_t n,
                                                           const int* __restrict__ tile_start, int* __restrict__ list) {
    __shared__ int cnt[kBlock];
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer;
    const int c = count_run(flag, n, b);
    cnt[threadIdx.x] = c;
    prg::scan_inclusive<kBlock>(cnt);
    int pos = tile_start[blockIdx.x] + cnt[threadIdx.x] - c;  // < the number of set flags whenever one is written
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u)
        if (b + u < n && flag[b + u] != 0) list[pos++] = (int)(b + u);
}

// the first `take` passing trials of the chunk become tuples have .. have + take - 1: three indices each, drawn again
__global__ __launch_bounds__(kBlock) void k_fgr_accept(const int* __restrict__ list, int64_t take, uint32_t C, uint64_t seed,
                                                       uint64_t t0, int64_t have, int* __restrict__ used) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= take) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) used[(have + i) * 3 + j] = (int)fg::draw(seed, t0 + (uint64_t)list[i], j, C);
}

// the used pairs in one array; an index outside the correspondences raises `bad` and reads nothing
__global__ __launch_bounds__(kBlock) void k_fgr_gather(const double* __restrict__ pq, int64_t C, const int* __restrict__ used,
                                                       int64_t K, double* __restrict__ upq, int* __restrict__ bad) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    const int64_t c = used[k];
    const bool ok = c >= 0 && c < C;
    if (!ok) bad[0] = 1;
#pragma unroll
    for (int a = 0; a < kPq; ++a) upq[k * kPq + a] = ok ? pq[c * kPq + a] : 0.0;
}

// ------------------------------------------------------------------------------------------------------------ optimise
// One run of kRun used pairs per lane, ascending k.  part: [run][kSlots].
__global__ __launch_bounds__(kBlock) void k_fgr_sums(const double* __restrict__ upq, int64_t K, const double* __restrict__ state,
                                                     double* __restrict__ part) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t k0 = r * fg::kRun;
    if (k0 >= K || state[kStStop] != 0.0) return;
    const int64_t k1 = k0 + fg::kRun < K ? k0 + fg::kRun : K;
    double pose[12], acc[fg::kSums];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = state[kStPose + k];
    const double mu = state[kStMu];
#pragma unroll
    for (int k = 0; k < fg::kSums; ++k) acc[k] = 0.0;
    for (int64_t k = k0; k < k1; ++k) {
        double p[3], q[3], c[fg::kSums];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[a] = upq[k * kPq + a];
            q[a] = upq[k * kPq + 3 + a];
        }
        fg::pair_terms(pose, mu, p, q, c);
#pragma unroll
        for (int s = 0; s < fg::kSums; ++s) acc[s] = fg::add(acc[s], c[s]);
    }
#pragma unroll
    for (int s = 0; s < fg::kSums; ++s) part[r * kSlots + s] = acc[s];
}

// One workgroup of kSlots lanes: lane s adds slot s of the runs in ascending run order into the state.
__global__ __launch_bounds__(kSlots) void k_fgr_total(const double* __restrict__ part, int64_t nruns, double* __restrict__ state) {
    if (state[kStStop] != 0.0 || (int)threadIdx.x >= fg::kSums) return;
    double acc = 0.0;
    int64_t r = 0;
    for (; r + 16 <= nruns; r += 16) {  // sixteen loads in flight; the additions stay in ascending run order
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = part[(r + u) * kSlots + threadIdx.x];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = fg::add(acc, v[u]);
    }
    for (; r < nruns; ++r) acc = fg::add(acc, part[r * kSlots + threadIdx.x]);
    state[kStSums + threadIdx.x] = acc;
}

// One lane.  The step from the sums in the state; a missing step (fewer than three pairs, a failed pivot) sets the stop flag
// and the status and leaves the pose and mu as they are.
__global__ void k_fgr_step(int64_t K, int decrease_mu, double division_factor, double max_corr_dist, double* __restrict__ state) {
    if (threadIdx.x != 0 || state[kStStop] != 0.0) return;
    double x[6];
    if (K < 3) {
        state[kStStop] = 1.0;
        state[kStStatus] = (double)kStatusTooFew;
        return;
    }
    if (!prg::cholesky6(state + kStSums, state + kStSums + 21, x)) {
        state[kStStop] = 1.0;
        state[kStStatus] = (double)kStatusDegenerate;
        return;
    }
    double d[12];
    prg::twist_to_pose(x, d);
    prg::compose_pose(d, state + kStPose);
    const int64_t i = (int64_t)state[kStIter];
    state[kStMu] = fg::next_mu(state[kStMu], i, decrease_mu != 0, division_factor, max_corr_dist);
    state[kStIter] = (double)(i + 1);
}

__global__ __launch_bounds__(kBlock) void k_fgr_weights(const double* __restrict__ upq, int64_t K, const double* __restrict__ state,
                                                        double* __restrict__ w) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    double pose[12], p[3], q[3];
#pragma unroll
    for (int a = 0; a < 12; ++a) pose[a] = state[kStPose + a];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = upq[k * kPq + a];
        q[a] = upq[k * kPq + 3 + a];
    }
    w[k] = fg::pair_weight(pose, state[kStMu], p, q);
}

// one lane: the state's pose in the caller's units
__global__ void k_fgr_denormalise(const double* __restrict__ state, const double* __restrict__ norm, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double pose[12], res[12];
    for (int k = 0; k < 12; ++k) pose[k] = state[kStPose + k];
    fg::denormalise(pose, norm + kNmMeanP, norm + kNmMeanQ, norm[kNmScaleGlobal], res);
    for (int k = 0; k < 12; ++k) out[k] = res[k];
}

}  // namespace

struct prg_fgr {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t M = 0, N = 0, C = 0, K = 0;
    bool have_pairs = false, have_used = false, have_state = false;
    int64_t chunk = kDefaultChunk;
    prg::DevBuf<double> src, tgt;            // [M][3], [N][3]
    prg::DevBuf<int> corr;                   // [C][2]
    prg::DevBuf<double> pq;                  // [C][kPq], normalised
    prg::DevBuf<double> mean_part, far_part; // the runs' sums and the workgroups' maxima of both clouds
    prg::DevBuf<double> norm, state, pose_out;
    prg::DevBuf<int> bad;
    prg::DevBuf<int> flag, list, tile_count, tile_start, n_list;  // one chunk of trials
    prg::DevBuf<int> used;                   // [K]
    prg::DevBuf<double> upq, part, wts;      // [K][kPq], [runs][kSlots], [K]
};

namespace {

int ensure_small(prg_fgr* h) {
    if (h->state.p) return PRG_OK;
    PRG_HIP(prg::reset_group(h->norm, (int64_t)kNmLen, h->state, (int64_t)kStLen, h->pose_out, (int64_t)12, h->bad, (int64_t)1,
                             h->n_list, (int64_t)1));
    return PRG_OK;
}

// `bad` was raised by a kernel: an index was out of range
int check_bad(prg_fgr* h, const char* who, const char* what) {
    int bad = 0;
    PRG_HIP(hipMemcpyAsync(&bad, h->bad.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_REQUIRE(bad == 0, PRG_ERR_INVALID, "%s: %s", who, what);
    return PRG_OK;
}

// upq <- the pairs used[0 .. K); sizes what depends on K.  Synchronises.
int gather_used(prg_fgr* h, const char* who, int64_t K) {
    hipStream_t st = h->stream;
    h->have_used = false;
    h->K = 0;
    const int64_t nruns = prg::ceil_div(K, fg::kRun);
    if (K > 0 && (h->upq.cap < K * kPq || h->part.cap < nruns * kSlots || h->wts.cap < K)) {
        PRG_HIP(hipStreamSynchronize(st));
        PRG_HIP(prg::reset_group(h->upq, K * kPq, h->part, nruns * kSlots, h->wts, K));
    }
    if (K > 0) {
        PRG_HIP(hipMemsetAsync(h->bad.p, 0, sizeof(int), st));
        k_fgr_gather<<<(unsigned)prg::ceil_div(K, kBlock), kBlock, 0, st>>>(h->pq.p, h->C, h->used.p, K, h->upq.p, h->bad.p);
        PRG_HIP(hipGetLastError());
        PRG_TRY(check_bad(h, who, "an index lies outside the correspondences"));
    }
    h->K = K;
    h->have_used = true;
    return PRG_OK;
}

void enqueue_sums(prg_fgr* h) {
    const int64_t nruns = prg::ceil_div(h->K, fg::kRun);
    if (nruns > 0) k_fgr_sums<<<(unsigned)prg::ceil_div(nruns, kBlock), kBlock, 0, h->stream>>>(h->upq.p, h->K, h->state.p, h->part.p);
    k_fgr_total<<<1, kSlots, 0, h->stream>>>(h->part.p, nruns, h->state.p);
}

int check_schedule(const char* who, double division_factor, double max_corr_dist) {
    PRG_REQUIRE(std::isfinite(division_factor) && division_factor > 1.0, PRG_ERR_INVALID,
                "%s: division_factor must be finite and > 1, got %g", who, division_factor);
    PRG_REQUIRE(std::isfinite(max_corr_dist) && max_corr_dist >= 0.0, PRG_ERR_INVALID,
                "%s: maximum_correspondence_distance must be finite and >= 0, got %g", who, max_corr_dist);
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_fgr_create(prg_fgr** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_fgr_destroy(prg_fgr* h) {
    return prg::destroy_handle(h);
}

int prg_fgr_set_clouds(prg_fgr* h, const double* source_hd, int64_t m, const double* target_hd, int64_t n) {
    PRG_REQUIRE(h && source_hd && target_hd, PRG_ERR_INVALID, "prg_fgr_set_clouds: NULL argument");
    PRG_REQUIRE(m >= 1 && n >= 1 && m < (int64_t)1 << 31 && n < (int64_t)1 << 31, PRG_ERR_INVALID,
                "prg_fgr_set_clouds: need 1 <= m, n < 2^31 points, got %lld and %lld", (long long)m, (long long)n);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->M = h->N = 0;
    h->have_pairs = h->have_used = h->have_state = false;
    PRG_TRY(ensure_small(h));
    const int64_t runs = prg::ceil_div(std::max(m, n), fg::kRun), blocks = prg::ceil_div(m, kBlock) + prg::ceil_div(n, kBlock);
    if (h->src.cap < m * 3 || h->tgt.cap < n * 3 || h->mean_part.cap < runs * kMeanSlots || h->far_part.cap < blocks)
        PRG_HIP(prg::reset_group(h->src, m * 3, h->tgt, n * 3, h->mean_part, runs * kMeanSlots, h->far_part, blocks));
    PRG_HIP(hipMemcpyAsync(h->src.p, source_hd, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(h->tgt.p, target_hd, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipStreamSynchronize(st));
    h->M = m;
    h->N = n;
    return PRG_OK;
}

int prg_fgr_set_correspondences(prg_fgr* h, const int* corr_hd, int64_t c) {
    PRG_REQUIRE(h && corr_hd, PRG_ERR_INVALID, "prg_fgr_set_correspondences: NULL argument");
    PRG_REQUIRE(c >= 3 && c <= ((int64_t)1 << 31) / fg::kTrialsPerPair, PRG_ERR_INVALID,
                "prg_fgr_set_correspondences: need 3 <= C <= 2^31 / %d correspondences, got %lld", fg::kTrialsPerPair, (long long)c);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->C = 0;
    h->have_pairs = h->have_used = false;
    if (h->corr.cap < c * 2 || h->pq.cap < c * kPq) PRG_HIP(prg::reset_group(h->corr, c * 2, h->pq, c * kPq));
    PRG_HIP(hipMemcpyAsync(h->corr.p, corr_hd, (size_t)c * 2 * sizeof(int), hipMemcpyDefault, st));
    PRG_HIP(hipStreamSynchronize(st));
    h->C = c;
    return PRG_OK;
}

int prg_fgr_normalise(prg_fgr* h, int use_absolute_scale, double* mean_p_host, double* mean_q_host, double* scale_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_normalise: NULL argument");
    PRG_REQUIRE(h->M >= 1, PRG_ERR_STATE, "prg_fgr_normalise: no clouds (prg_fgr_set_clouds first)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    h->have_pairs = h->have_used = false;
    const double* cloud[2] = {h->src.p, h->tgt.p};
    const int64_t rows[2] = {h->M, h->N};
    const int64_t nb0 = prg::ceil_div(h->M, kBlock), nb1 = prg::ceil_div(h->N, kBlock);
    for (int w = 0; w < 2; ++w) {
        const int64_t nruns = prg::ceil_div(rows[w], fg::kRun);
        k_fgr_run_sums<<<(unsigned)prg::ceil_div(nruns, kBlock), kBlock, 0, st>>>(cloud[w], rows[w], h->mean_part.p);
        k_fgr_mean<<<1, kMeanSlots, 0, st>>>(h->mean_part.p, nruns, rows[w], h->norm.p + (w == 0 ? kNmMeanP : kNmMeanQ));
        k_fgr_far<<<(unsigned)(w == 0 ? nb0 : nb1), kBlock, 0, st>>>(cloud[w], rows[w], h->norm.p + (w == 0 ? kNmMeanP : kNmMeanQ),
                                                                   h->far_part.p + (w == 0 ? 0 : nb0));
    }
    k_fgr_scale<<<1, kBlock, 0, st>>>(h->far_part.p, nb0 + nb1, use_absolute_scale, h->norm.p);
    PRG_HIP(hipGetLastError());
    double norm[kNmLen];
    PRG_HIP(hipMemcpyAsync(norm, h->norm.p, sizeof(norm), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    for (int a = 0; a < 3; ++a) {
        if (mean_p_host) mean_p_host[a] = norm[kNmMeanP + a];
        if (mean_q_host) mean_q_host[a] = norm[kNmMeanQ + a];
    }
    if (scale_host) *scale_host = norm[kNmScale];
    if (h->C >= 3 && norm[kNmScaleGlobal] > 0.0 && std::isfinite(norm[kNmScaleGlobal])) {
        PRG_HIP(hipMemsetAsync(h->bad.p, 0, sizeof(int), st));
        k_fgr_pack<<<(unsigned)prg::ceil_div(h->C, kBlock), kBlock, 0, st>>>(h->src.p, h->M, h->tgt.p, h->N, h->corr.p, h->C,
                                                                            h->norm.p, h->pq.p, h->bad.p);
        PRG_HIP(hipGetLastError());
        PRG_TRY(check_bad(h, "prg_fgr_normalise", "a correspondence indexes outside the clouds"));
        h->have_pairs = true;
    }
    return PRG_OK;
}

int prg_fgr_set_chunk(prg_fgr* h, int64_t trials) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_set_chunk: NULL argument");
    PRG_REQUIRE(trials >= 0 && trials <= kMaxChunk, PRG_ERR_INVALID, "prg_fgr_set_chunk: trials must lie in 0 .. %lld, got %lld",
                (long long)kMaxChunk, (long long)trials);
    h->chunk = trials == 0 ? kDefaultChunk : trials;
    return PRG_OK;
}

int prg_fgr_tuples(prg_fgr* h, uint64_t seed, double tuple_scale, int64_t maximum_tuple_count, int64_t* n_tuples_host,
                   int64_t* n_trials_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_tuples: NULL argument");
    PRG_REQUIRE(tuple_scale > 0.0 && tuple_scale <= 1.0, PRG_ERR_INVALID, "prg_fgr_tuples: tuple_scale must lie in (0, 1], got %g",
                tuple_scale);
    PRG_REQUIRE(maximum_tuple_count >= 1 && maximum_tuple_count <= kMaxTuples, PRG_ERR_INVALID,
                "prg_fgr_tuples: maximum_tuple_count must lie in 1 .. %lld, got %lld", (long long)kMaxTuples,
                (long long)maximum_tuple_count);
    PRG_REQUIRE(h->have_pairs, PRG_ERR_STATE,
                "prg_fgr_tuples: no normalised pairs (prg_fgr_set_correspondences, then prg_fgr_normalise with a scale > 0)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->have_used = false;
    const int64_t cap = maximum_tuple_count, limit = fg::kTrialsPerPair * h->C, chunk = std::min(h->chunk, limit);
    const int ntiles = (int)prg::ceil_div(chunk, kCompactTile);
    if (h->flag.cap < chunk || h->list.cap < chunk || h->tile_count.cap < ntiles || h->tile_start.cap < ntiles)
        PRG_HIP(prg::reset_group(h->flag, chunk, h->list, chunk, h->tile_count, (int64_t)ntiles, h->tile_start, (int64_t)ntiles));
    PRG_HIP(h->used.ensure(cap * 3, cap * 3));
    int64_t have = 0, n_trials = limit;
    for (int64_t t0 = 0; t0 < limit && have < cap; t0 += chunk) {
        const int64_t n = std::min(chunk, limit - t0);
        const int nt = (int)prg::ceil_div(n, kCompactTile);
        k_fgr_trials<<<(unsigned)prg::ceil_div(n, kBlock), kBlock, 0, st>>>(h->pq.p, (uint32_t)h->C, seed, (uint64_t)t0, n,
                                                                           tuple_scale, h->flag.p);
        k_fgr_flag_count<<<nt, kBlock, 0, st>>>(h->flag.p, n, h->tile_count.p);
        k_fgr_tile_scan<<<1, kScanThreads, 0, st>>>(h->tile_count.p, nt, h->tile_start.p, h->n_list.p);
        k_fgr_flag_write<<<nt, kBlock, 0, st>>>(h->flag.p, n, h->tile_start.p, h->list.p);
        PRG_HIP(hipGetLastError());
        int n_pass = 0;
        PRG_HIP(hipMemcpyAsync(&n_pass, h->n_list.p, sizeof(int), hipMemcpyDeviceToHost, st));
        PRG_HIP(hipStreamSynchronize(st));
        const int64_t take = std::min<int64_t>(n_pass, cap - have);
        if (take <= 0) continue;
        k_fgr_accept<<<(unsigned)prg::ceil_div(take, kBlock), kBlock, 0, st>>>(h->list.p, take, (uint32_t)h->C, seed, (uint64_t)t0,
                                                                              have, h->used.p);
        PRG_HIP(hipGetLastError());
        have += take;
        if (have == cap) {
            int last = 0;
            PRG_HIP(hipMemcpyAsync(&last, h->list.p + (take - 1), sizeof(int), hipMemcpyDeviceToHost, st));
            PRG_HIP(hipStreamSynchronize(st));
            n_trials = t0 + last + 1;
        }
    }
    PRG_TRY(gather_used(h, "prg_fgr_tuples", have * 3));
    if (n_tuples_host) *n_tuples_host = have;
    if (n_trials_host) *n_trials_host = n_trials;
    return PRG_OK;
}

int prg_fgr_set_used(prg_fgr* h, const int* index_hd, int64_t k) {
    PRG_REQUIRE(h && (index_hd || k == 0), PRG_ERR_INVALID, "prg_fgr_set_used: NULL argument");
    PRG_REQUIRE(k >= 0 && k <= 3 * kMaxTuples, PRG_ERR_INVALID, "prg_fgr_set_used: need 0 <= K <= %lld indices, got %lld",
                (long long)(3 * kMaxTuples), (long long)k);
    PRG_REQUIRE(h->have_pairs, PRG_ERR_STATE,
                "prg_fgr_set_used: no normalised pairs (prg_fgr_set_correspondences, then prg_fgr_normalise with a scale > 0)");
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_used = false;
    PRG_HIP(h->used.ensure(k, k));
    if (k > 0) PRG_TRY(prg::copy_in(h->used, index_hd, k, h->stream));
    return gather_used(h, "prg_fgr_set_used", k);
}

int prg_fgr_get_used(prg_fgr* h, int* index_host) {
    PRG_REQUIRE(h && index_host, PRG_ERR_INVALID, "prg_fgr_get_used: NULL argument");
    PRG_REQUIRE(h->have_used, PRG_ERR_STATE, "prg_fgr_get_used: prg_fgr_tuples or prg_fgr_set_used first");
    PRG_ENTER(h->device);
    if (h->K > 0) PRG_TRY(prg::copy_out(index_host, h->used, h->K, h->stream));
    return PRG_OK;
}

int prg_fgr_set_state(prg_fgr* h, const double* pose_host, double mu) {
    PRG_REQUIRE(h && pose_host, PRG_ERR_INVALID, "prg_fgr_set_state: NULL argument");
    for (int k = 0; k < 12; ++k)
        PRG_REQUIRE(std::isfinite(pose_host[k]), PRG_ERR_INVALID, "prg_fgr_set_state: the pose contains NaN or infinity");
    PRG_REQUIRE(std::isfinite(mu) && mu > 0.0, PRG_ERR_INVALID, "prg_fgr_set_state: mu must be finite and > 0, got %g", mu);
    PRG_ENTER(h->device);
    PRG_TRY(ensure_small(h));
    double state[kStLen] = {0.0};
    for (int k = 0; k < 12; ++k) state[kStPose + k] = pose_host[k];
    state[kStMu] = mu;
    state[kStStatus] = (double)kStatusOk;
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(hipMemcpy(h->state.p, state, sizeof(state), hipMemcpyHostToDevice));
    h->have_state = true;
    return PRG_OK;
}

int prg_fgr_sums(prg_fgr* h, double* sums_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_sums: NULL argument");
    PRG_REQUIRE(h->have_used && h->have_state, PRG_ERR_STATE, "prg_fgr_sums: needs the used pairs and a state (prg_fgr_tuples or "
                "prg_fgr_set_used, and prg_fgr_set_state)");
    PRG_ENTER(h->device);
    enqueue_sums(h);
    PRG_HIP(hipGetLastError());
    PRG_TRY(prg::copy_out(sums_host, h->state, fg::kSums, h->stream, kStSums));
    return PRG_OK;
}

int prg_fgr_step(prg_fgr* h, int decrease_mu, double division_factor, double maximum_correspondence_distance) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_step: NULL argument");
    PRG_TRY(check_schedule("prg_fgr_step", division_factor, maximum_correspondence_distance));
    PRG_REQUIRE(h->have_used && h->have_state, PRG_ERR_STATE, "prg_fgr_step: prg_fgr_sums first");
    PRG_ENTER(h->device);
    k_fgr_step<<<1, 1, 0, h->stream>>>(h->K, decrease_mu, division_factor, maximum_correspondence_distance, h->state.p);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int prg_fgr_iterate(prg_fgr* h, int iterations, int decrease_mu, double division_factor, double maximum_correspondence_distance) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_iterate: NULL argument");
    PRG_REQUIRE(iterations >= 0 && iterations <= 100000, PRG_ERR_INVALID,
                "prg_fgr_iterate: iterations must lie in 0 .. 100000, got %d", iterations);
    PRG_TRY(check_schedule("prg_fgr_iterate", division_factor, maximum_correspondence_distance));
    PRG_REQUIRE(h->have_used && h->have_state, PRG_ERR_STATE, "prg_fgr_iterate: needs the used pairs and a state (prg_fgr_tuples "
                "or prg_fgr_set_used, and prg_fgr_set_state)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    for (int i0 = 0; i0 < iterations; i0 += kIterChunk) {
        for (int i = i0; i < std::min(iterations, i0 + kIterChunk); ++i) {
            enqueue_sums(h);
            k_fgr_step<<<1, 1, 0, st>>>(h->K, decrease_mu, division_factor, maximum_correspondence_distance, h->state.p);
        }
        PRG_HIP(hipGetLastError());
        if (i0 + kIterChunk >= iterations) break;
        double stop = 0.0;  // once per chunk: a stopped loop needs no further launches
        PRG_HIP(hipMemcpyAsync(&stop, h->state.p + kStStop, sizeof(double), hipMemcpyDeviceToHost, st));
        PRG_HIP(hipStreamSynchronize(st));
        if (stop != 0.0) break;
    }
    return PRG_OK;
}

int prg_fgr_get_state(prg_fgr* h, int caller_units, double* pose_host, double* mu_host, int64_t* n_iter_host, int* status_host,
                      double* objective_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fgr_get_state: NULL argument");
    PRG_REQUIRE(h->have_state, PRG_ERR_STATE, "prg_fgr_get_state: prg_fgr_set_state first");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    double state[kStLen], pose[12];
    if (caller_units) {
        k_fgr_denormalise<<<1, 1, 0, st>>>(h->state.p, h->norm.p, h->pose_out.p);
        PRG_HIP(hipGetLastError());
        PRG_HIP(hipMemcpyAsync(pose, h->pose_out.p, sizeof(pose), hipMemcpyDeviceToHost, st));
    }
    PRG_HIP(hipMemcpyAsync(state, h->state.p, sizeof(state), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    if (pose_host)
        for (int k = 0; k < 12; ++k) pose_host[k] = caller_units ? pose[k] : state[kStPose + k];
    if (mu_host) *mu_host = state[kStMu];
    if (n_iter_host) *n_iter_host = (int64_t)state[kStIter];
    if (status_host) *status_host = (int)state[kStStatus];
    if (objective_host) *objective_host = state[kStSums + fg::kSums - 1];
    return PRG_OK;
}

int prg_fgr_get_weights(prg_fgr* h, double* weights_host) {
    PRG_REQUIRE(h && weights_host, PRG_ERR_INVALID, "prg_fgr_get_weights: NULL argument");
    PRG_REQUIRE(h->have_used && h->have_state, PRG_ERR_STATE, "prg_fgr_get_weights: needs the used pairs and a state");
    PRG_ENTER(h->device);
    if (h->K == 0) return PRG_OK;
    k_fgr_weights<<<(unsigned)prg::ceil_div(h->K, kBlock), kBlock, 0, h->stream>>>(h->upq.p, h->K, h->state.p, h->wts.p);
    PRG_HIP(hipGetLastError());
    PRG_TRY(prg::copy_out(weights_host, h->wts, h->K, h->stream));
    return PRG_OK;
}

}  // extern "C"
