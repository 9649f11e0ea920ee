// Global registration: a start pose for the local methods from matched descriptors, all in fp64 with
// fixed-order sums and no floating-point atomics.
//
//   prg_feature_match[_mutual]  all-pairs nearest descriptor: one owned row per lane with its d values in registers, the other
//                               side streamed wave-uniformly (scalar loads) in segments, per-segment minima merged in order
//   prg_ransac_*                hypotheses (splitmix64 triples, Open3D's edge-length check, three-point Kabsch), the scoring
//                               sweep "hypotheses x correspondences", the winner by (count, sum, h), refits on the inliers
//
// Every discrete result (match index, triple, validity flag, inlier count, winner) is a function of the input alone: the
// matching minimum is exact under any cut, the scoring sum is cut into segments of kScoreSegment correspondences whatever
// the launch, the refit's sums into runs of kRefitRun.
#include <algorithm>
#include <cmath>
#include <new>

#include "block_scan.h"
#include "dev_buf.h"
#include "kabsch_pose.h"
#include "prg_common.h"
#include "small_linalg.h"

namespace {

using prg::kabsch_pose;

constexpr int kBlock = 256;
constexpr int kMaxDim = 64;
constexpr int kMaxSegments = 4096;
constexpr int kScoreSegment = 1024;      // correspondences per segment of a hypothesis' ordered sum (part of the definition)
constexpr int kRefitRun = 64;            // correspondences per run of the refit's sums (part of the definition)
constexpr int64_t kScoreBatch = 65536;   // hypotheses per scoring launch: bounds the partial buffers, not the result
constexpr int64_t kMaxHyp = (int64_t)1 << 24;
constexpr int kBestThreads = 1024;
constexpr int kCompactPer = 16;                      // flags per lane of the compaction
constexpr int kCompactTile = kBlock * kCompactPer;   // hypotheses per workgroup of the compaction
constexpr double kDegenerate = 0.05;
constexpr int kPq = 8;                   // doubles per packed correspondence: P, Q, two pads (one 64-byte scalar load)

// ------------------------------------------------------------------------------------------------------------ matching
// rows [n][d] -> [n][D], zero-filled behind d: (0 - 0)^2 adds an exact 0 to D^2, so the pad changes no bit of it
__global__ __launch_bounds__(kBlock) void k_pad_rows(const double* __restrict__ in, int64_t n, int d, int D,
                                                     double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= n * D) return;
    const int64_t r = e / D;
    const int k = (int)(e - r * D);
    out[e] = k < d ? in[r * d + k] : 0.0;
}

// D^2 of the owned row in registers and one streamed row, k ascending, every operation rounded once
template <int D>
__device__ __forceinline__ double dist2(const double (&a)[D], const double* __restrict__ b) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double diff = __dsub_rn(a[k], b[k]);
        acc = __dadd_rn(acc, __dmul_rn(diff, diff));
    }
    return acc;
}

// Lane i owns row i; the workgroup streams segment blockIdx.y = [y seg_len, min((y + 1) seg_len, n_s)) of the other side.
// Nothing past n_s is read.  part_d2 / part_idx: [segment][n_o].  Strict "<" on ascending j: ties keep the smaller index.
template <int D>
__global__ __launch_bounds__(kBlock) void k_feature_match(const double* __restrict__ own, int64_t n_o,
                                                          const double* __restrict__ str, int64_t n_s, int64_t seg_len,
                                                          double* __restrict__ part_d2, int* __restrict__ part_idx) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t ii = i < n_o ? i : n_o - 1;  // lanes past the end redo the last row and store nothing
    double a[D];
#pragma unroll
    for (int k = 0; k < D; ++k) a[k] = own[ii * D + k];
    const int64_t j0 = (int64_t)blockIdx.y * seg_len;
    const int64_t j1 = j0 + seg_len < n_s ? j0 + seg_len : n_s;
    double best = INFINITY;
    int bi = -1;
    int64_t j = j0;
    for (; j + 2 <= j1; j += 2) {  // two independent chains of D dependent additions
        const double v0 = dist2<D>(a, str + j * D);
        const double v1 = dist2<D>(a, str + (j + 1) * D);
        if (v0 < best || bi < 0) { best = v0; bi = (int)j; }
        if (v1 < best) { best = v1; bi = (int)(j + 1); }
    }
    for (; j < j1; ++j) {
        const double v = dist2<D>(a, str + j * D);
        if (v < best || bi < 0) { best = v; bi = (int)j; }
    }
    if (i < n_o) {
        part_d2[(int64_t)blockIdx.y * n_o + i] = best;
        part_idx[(int64_t)blockIdx.y * n_o + i] = bi;
    }
}

// minimum over the segments in ascending segment order (= ascending index): strict "<" keeps the smaller index
__global__ __launch_bounds__(kBlock) void k_match_merge(const double* __restrict__ part_d2, const int* __restrict__ part_idx,
                                                        int nseg, int64_t n_o, int* __restrict__ idx_out,
                                                        double* __restrict__ d2_out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_o) return;
    double best = part_d2[i];
    int bi = part_idx[i];
    for (int g = 1; g < nseg; ++g) {
        const double v = part_d2[(int64_t)g * n_o + i];
        const int id = part_idx[(int64_t)g * n_o + i];
        if (id >= 0 && (v < best || bi < 0)) { best = v; bi = id; }
    }
    idx_out[i] = bi;
    d2_out[i] = best;
}

// pair (a, ab[a]) stays iff a is the best row for ab[a] as well
__global__ __launch_bounds__(kBlock) void k_mutual(const int* __restrict__ ab, const int* __restrict__ ba, int64_t na,
                                                   int64_t nb, int* __restrict__ keep) {
    const int64_t a = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (a >= na) return;
    const int b = ab[a];
    keep[a] = (b >= 0 && b < nb && ba[b] == (int)a) ? 1 : 0;
}

int template_dim(int d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 33 ? 33 : d <= 48 ? 48 : 64; }

// segments of the streamed side: (count, length); automatic as the top-k sweep cuts its own (enough workgroups to fill the chip)
void cut_segments(int64_t n_o, int64_t n_s, int segments, int* nseg, int64_t* seg_len) {
    int64_t want = segments;
    if (want <= 0) {
        const int64_t nbx = prg::ceil_div(n_o, kBlock);
        want = std::min<int64_t>(std::max<int64_t>(1, 2048 / nbx), prg::ceil_div(n_s, 256));
    }
    want = std::min<int64_t>(want, n_s);
    *seg_len = prg::ceil_div(n_s, want);
    *nseg = (int)prg::ceil_div(n_s, *seg_len);  // no empty segment
}

// own / str: padded rows [n][D] on the device -> idx_dev / d2_dev [n_o].  Enqueues only.
int run_match(hipStream_t st, int D, const double* own, int64_t n_o, const double* str, int64_t n_s, int segments,
              prg::DevBuf<double>& part_d2, prg::DevBuf<int>& part_idx, int* idx_dev, double* d2_dev) {
    int nseg;
    int64_t seg_len;
    cut_segments(n_o, n_s, segments, &nseg, &seg_len);
    PRG_HIP(part_d2.ensure((int64_t)nseg * n_o, (int64_t)nseg * n_o));
    PRG_HIP(part_idx.ensure((int64_t)nseg * n_o, (int64_t)nseg * n_o));
    const dim3 grid((unsigned)prg::ceil_div(n_o, kBlock), (unsigned)nseg);
#define PRG_MATCH_LAUNCH(DD) \
    k_feature_match<DD><<<grid, kBlock, 0, st>>>(own, n_o, str, n_s, seg_len, part_d2.p, part_idx.p)
    switch (D) {
        case 8: PRG_MATCH_LAUNCH(8); break;
        case 16: PRG_MATCH_LAUNCH(16); break;
        case 33: PRG_MATCH_LAUNCH(33); break;
        case 48: PRG_MATCH_LAUNCH(48); break;
        default: PRG_MATCH_LAUNCH(64); break;
    }
#undef PRG_MATCH_LAUNCH
    k_match_merge<<<grid.x, kBlock, 0, st>>>(part_d2.p, part_idx.p, nseg, n_o, idx_dev, d2_dev);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int match_impl(const char* who, int device, void* hip_stream, const double* a_hd, int64_t na, const double* b_hd, int64_t nb,
               int d, int segments, int* idx_out, double* d2_out, int* mutual_out) {
    PRG_REQUIRE(a_hd && b_hd && idx_out && d2_out, PRG_ERR_INVALID, "%s: NULL argument", who);
    PRG_REQUIRE(d >= 1 && d <= kMaxDim, PRG_ERR_INVALID, "%s: d must lie in 1 .. %d, got %d", who, kMaxDim, d);
    PRG_REQUIRE(na >= 1 && nb >= 1 && na < (int64_t)1 << 31 && nb < (int64_t)1 << 31, PRG_ERR_INVALID,
                "%s: need 1 <= na, nb < 2^31", who);
    PRG_REQUIRE(segments >= 0 && segments <= kMaxSegments, PRG_ERR_INVALID, "%s: segments must lie in 0 .. %d", who,
                kMaxSegments);
    PRG_ENTER_AS(who, device);
    hipStream_t st = (hipStream_t)hip_stream;
    const int D = template_dim(d);
    prg::DevBuf<double> raw, a_pad, b_pad, part_d2, d2_ab, d2_ba;
    prg::DevBuf<int> part_idx, idx_ab, idx_ba, keep;
    PRG_HIP(raw.reset(std::max(na, nb) * d));
    PRG_HIP(a_pad.reset(na * D));
    PRG_HIP(b_pad.reset(nb * D));
    PRG_HIP(idx_ab.reset(na));
    PRG_HIP(d2_ab.reset(na));
    PRG_HIP(hipMemcpyAsync(raw.p, a_hd, (size_t)na * d * sizeof(double), hipMemcpyDefault, st));
    k_pad_rows<<<(unsigned)prg::ceil_div(na * D, kBlock), kBlock, 0, st>>>(raw.p, na, d, D, a_pad.p);
    PRG_HIP(hipMemcpyAsync(raw.p, b_hd, (size_t)nb * d * sizeof(double), hipMemcpyDefault, st));
    k_pad_rows<<<(unsigned)prg::ceil_div(nb * D, kBlock), kBlock, 0, st>>>(raw.p, nb, d, D, b_pad.p);
    PRG_HIP(hipGetLastError());
    PRG_TRY(run_match(st, D, a_pad.p, na, b_pad.p, nb, segments, part_d2, part_idx, idx_ab.p, d2_ab.p));
    if (mutual_out) {
        PRG_HIP(idx_ba.reset(nb));
        PRG_HIP(d2_ba.reset(nb));
        PRG_HIP(keep.reset(na));
        PRG_HIP(hipStreamSynchronize(st));  // the partial lists may be re-created for the other direction
        PRG_TRY(run_match(st, D, b_pad.p, nb, a_pad.p, na, segments, part_d2, part_idx, idx_ba.p, d2_ba.p));
        k_mutual<<<(unsigned)prg::ceil_div(na, kBlock), kBlock, 0, st>>>(idx_ab.p, idx_ba.p, na, nb, keep.p);
        PRG_HIP(hipGetLastError());
        PRG_HIP(hipMemcpyAsync(mutual_out, keep.p, (size_t)na * sizeof(int), hipMemcpyDefault, st));
    }
    PRG_HIP(hipMemcpyAsync(idx_out, idx_ab.p, (size_t)na * sizeof(int), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(d2_out, d2_ab.p, (size_t)na * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

// ---------------------------------------------------------------------------------------------------------- hypotheses
__device__ __forceinline__ uint64_t splitmix64(uint64_t seed, uint64_t counter) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * counter;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// One hypothesis per lane: the draw, the three checks, the three-point Kabsch.  pq: [C][kPq].
__global__ __launch_bounds__(kBlock) void k_hyp_build(const double* __restrict__ pq, uint32_t C, uint64_t seed,
                                                      uint64_t h_offset, int64_t H, double s, int* __restrict__ tri,
                                                      double* __restrict__ pose, int* __restrict__ valid) {
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    uint32_t id[3];
    double p[3][3], q[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint64_t z = splitmix64(seed, 3ull * (h_offset + (uint64_t)h) + (uint64_t)j + 1ull);
        id[j] = (uint32_t)(((z >> 32) * (uint64_t)C) >> 32);  // < C
        tri[h * 3 + j] = (int)id[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            p[j][a] = pq[(int64_t)id[j] * kPq + a];
            q[j][a] = pq[(int64_t)id[j] * kPq + 3 + a];
        }
    }
    bool ok = id[0] != id[1] && id[1] != id[2] && id[0] != id[2];
    constexpr int ea[3] = {0, 0, 1}, eb[3] = {1, 2, 2};
#pragma unroll
    for (int e = 0; e < 3; ++e) {
        const double lp = norm3(p[eb[e]][0] - p[ea[e]][0], p[eb[e]][1] - p[ea[e]][1], p[eb[e]][2] - p[ea[e]][2]);
        const double lq = norm3(q[eb[e]][0] - q[ea[e]][0], q[eb[e]][1] - q[ea[e]][1], q[eb[e]][2] - q[ea[e]][2]);
        ok = ok && lp >= s * lq && lq >= s * lp;
    }
    const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    ok = ok && norm3(cx, cy, cz) >= kDegenerate * norm3(e1[0], e1[1], e1[2]) * norm3(e2[0], e2[1], e2[2]);
    double out[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = 0.0;
    if (ok) {
        double pm[3], qm[3], hm[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            pm[a] = (p[0][a] + p[1][a] + p[2][a]) / 3.0;
            qm[a] = (q[0][a] + q[1][a] + q[2][a]) / 3.0;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 3; ++j) acc += (p[j][a] - pm[a]) * (q[j][b] - qm[b]);
                hm[a][b] = acc;
            }
        kabsch_pose(hm, pm, qm, out);
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[h * 12 + k] = out[k];
    valid[h] = ok ? 1 : 0;
}

// r^2 = |R p + t - q|^2 in the order the definition writes it, every operation rounded once (no contraction): component a is
// (((R_a0 p_x + R_a1 p_y) + R_a2 p_z) + t_a) - q_a, then (r_x^2 + r_y^2) + r_z^2 - so that a plain IEEE restatement gets the
// same bits, the inlier decision and the ordered sums included.
__device__ __forceinline__ double resid1(double r0, double r1, double r2, double t, const double* __restrict__ c, int a) {
    const double s = __dadd_rn(__dadd_rn(__dmul_rn(r0, c[0]), __dmul_rn(r1, c[1])), __dmul_rn(r2, c[2]));
    return __dsub_rn(__dadd_rn(s, t), c[3 + a]);
}
__device__ __forceinline__ double resid2(const double (&m)[12], const double* __restrict__ c) {
    const double rx = resid1(m[0], m[1], m[2], m[9], c, 0);
    const double ry = resid1(m[3], m[4], m[5], m[10], c, 1);
    const double rz = resid1(m[6], m[7], m[8], m[11], c, 2);
    return __dadd_rn(__dadd_rn(__dmul_rn(rx, rx), __dmul_rn(ry, ry)), __dmul_rn(rz, rz));
}

// The indices of the valid hypotheses in ascending order, in three small launches: valid flags per tile of kCompactTile
// hypotheses, an exclusive scan over the tiles (one workgroup), the order-preserving write.  The scoring sweep then holds a
// valid hypothesis in every lane, however few of the draws passed the checks.  A lane looks at kCompactPer consecutive flags.
__device__ __forceinline__ int count_run(const int* __restrict__ valid, int64_t H, int64_t b) {
    int c = 0;
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u) c += (b + u < H && valid[b + u < H ? b + u : 0] != 0) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(kBlock) void k_valid_count(const int* __restrict__ valid, int64_t H, int* __restrict__ tile_count) {
    __shared__ int cnt[kBlock];
    cnt[threadIdx.x] = count_run(valid, H, ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer);
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

__global__ __launch_bounds__(kBlock) void k_valid_write(const int* __restrict__ valid, int64_t H, const int* __restrict__ tile_start,
                                                        int* __restrict__ list) {
    __shared__ int cnt[kBlock];
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCompactPer;
    const int c = count_run(valid, H, b);
    cnt[threadIdx.x] = c;
    prg::scan_inclusive<kBlock>(cnt);
    int pos = tile_start[blockIdx.x] + cnt[threadIdx.x] - c;  // < the number of valid hypotheses whenever one is written
#pragma unroll
    for (int u = 0; u < kCompactPer; ++u)
        if (b + u < H && valid[b + u] != 0) list[pos++] = (int)(b + u);
}

// what an invalid hypothesis reports: (-1, 0); the valid ones are overwritten by k_score_merge
__global__ __launch_bounds__(kBlock) void k_score_fill(int64_t H, int* __restrict__ counts, double* __restrict__ sums) {
    const int64_t h = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (h >= H) return;
    counts[h] = -1;
    sums[h] = 0.0;
}

// One valid hypothesis per lane (list[0 .. n_l) of this launch) with its 12 doubles in registers; the workgroup streams segment
// blockIdx.y of the correspondences wave-uniformly.  part_*: [segment][n_l].
__global__ __launch_bounds__(kBlock) void k_hyp_score(const double* __restrict__ pq, int64_t C,
                                                      const double* __restrict__ pose, const int* __restrict__ list,
                                                      int64_t n_l, double tau2, int* __restrict__ part_count,
                                                      double* __restrict__ part_sum) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t h = list[l < n_l ? l : n_l - 1];  // lanes past the end redo the last hypothesis and store nothing
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = pose[h * 12 + k];
    int cnt = 0;
    double sum = 0.0;
    const int64_t c0 = (int64_t)blockIdx.y * kScoreSegment;
    const int64_t c1 = c0 + kScoreSegment < C ? c0 + kScoreSegment : C;
    for (int64_t c = c0; c < c1; ++c) {
        const double r2 = resid2(m, pq + c * kPq);
        const bool in = r2 <= tau2;
        cnt += in ? 1 : 0;
        sum += in ? r2 : 0.0;  // + 0.0 is exact: the sum runs over the inliers in ascending c
    }
    if (l < n_l) {
        part_count[(int64_t)blockIdx.y * n_l + l] = cnt;
        part_sum[(int64_t)blockIdx.y * n_l + l] = sum;
    }
}

// segment results in ascending segment order, stored at the hypothesis' own index
__global__ __launch_bounds__(kBlock) void k_score_merge(const int* __restrict__ part_count, const double* __restrict__ part_sum,
                                                        int nseg, const int* __restrict__ list, int64_t n_l,
                                                        int* __restrict__ counts, double* __restrict__ sums) {
    const int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (l >= n_l) return;
    int cnt = 0;
    double sum = 0.0;
    for (int g = 0; g < nseg; ++g) {
        cnt += part_count[(int64_t)g * n_l + l];
        sum += part_sum[(int64_t)g * n_l + l];
    }
    counts[list[l]] = cnt;
    sums[list[l]] = sum;
}

// (count, sum, h) is a strict total order, so the winner does not depend on how the reduction is shaped
__device__ __forceinline__ bool ranks_ahead(int ca, double sa, int ha, int cb, double sb, int hb) {
    if (ca != cb) return ca > cb;
    if (sa != sb) return sa < sb;
    return ha < hb;
}

// one workgroup over the valid hypotheses: best_i = (h or -1, count), best_d = (sum, pose[12])
__global__ __launch_bounds__(kBestThreads) void k_best(const int* __restrict__ counts, const double* __restrict__ sums,
                                                       const double* __restrict__ pose, const int* __restrict__ list,
                                                       int64_t n_valid, int* __restrict__ best_i, double* __restrict__ best_d) {
    __shared__ int sc[kBestThreads], sh[kBestThreads];
    __shared__ double ss[kBestThreads];
    int bc = -1, bh = 0x7fffffff;
    double bs = INFINITY;
    for (int64_t l = threadIdx.x; l < n_valid; l += kBestThreads) {
        const int64_t h = list[l];
        const int c = counts[h];
        const double s = sums[h];
        if (c >= 0 && ranks_ahead(c, s, (int)h, bc, bs, bh)) { bc = c; bs = s; bh = (int)h; }
    }
    sc[threadIdx.x] = bc; ss[threadIdx.x] = bs; sh[threadIdx.x] = bh;
    __syncthreads();
    for (int w = kBestThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const int o = threadIdx.x + w;
            if (sc[o] >= 0 && ranks_ahead(sc[o], ss[o], sh[o], sc[threadIdx.x], ss[threadIdx.x], sh[threadIdx.x])) {
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
        for (int k = 0; k < 12; ++k) best_d[1 + k] = any ? pose[(int64_t)sh[0] * 12 + k] : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------- refit
// state (doubles): [0, 12) pose, [12, 18) centroids of the inliers (P, Q), [18] stop (fewer than 3 inliers), [19] count, [20] sum
constexpr int kStatePose = 0, kStateCentre = 12, kStateStop = 18, kStateCount = 19, kStateSum = 20, kStateLen = 24;
constexpr int kRefitSlots = 16;
// mode 0: run sums of (count, r^2, P, Q) over the inliers of state's pose; mode 1: of the centred products (P - pm)(Q - qm)^T.
// One run of kRefitRun correspondences per lane, ascending c.  part: [run][kRefitSlots].  inl (may be null): the inlier flags.
__global__ __launch_bounds__(kBlock) void k_refit_sums(const double* __restrict__ pq, int64_t C, const double* __restrict__ state,
                                                       double tau2, int mode, double* __restrict__ part, int* __restrict__ inl) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t c0 = r * kRefitRun;
    if (c0 >= C) return;
    const int64_t c1 = c0 + kRefitRun < C ? c0 + kRefitRun : C;
    double m[12], ctr[6], acc[kRefitSlots];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = state[kStatePose + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) ctr[k] = state[kStateCentre + k];
#pragma unroll
    for (int k = 0; k < kRefitSlots; ++k) acc[k] = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        const double* __restrict__ e = pq + c * kPq;
        const double r2 = resid2(m, e);
        const bool in = r2 <= tau2;
        if (inl) inl[c] = in ? 1 : 0;
        if (!in) continue;
        acc[0] += 1.0;
        acc[1] += r2;
        if (mode == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) acc[2 + k] += e[k];
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) acc[2 + 3 * a + b] += (e[a] - ctr[a]) * (e[3 + b] - ctr[3 + b]);
        }
    }
#pragma unroll
    for (int k = 0; k < kRefitSlots; ++k) part[r * kRefitSlots + k] = acc[k];
}

// One workgroup of kRefitSlots lanes: lane k adds slot k of the runs in ascending run order; lane 0 then finishes the step.
// mode 0: centroids (or stop); mode 1: Kabsch on the centred products -> new pose (unless stopped); mode 2: count and sum.
__global__ __launch_bounds__(kRefitSlots) void k_refit_step(const double* __restrict__ part, int64_t nruns, int mode,
                                                            double* __restrict__ state) {
    __shared__ double tot[kRefitSlots];
    double acc = 0.0;
    int64_t r = 0;
    for (; r + 8 <= nruns; r += 8) {  // eight loads in flight; the additions stay in ascending run order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(r + u) * kRefitSlots + threadIdx.x];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; r < nruns; ++r) acc += part[r * kRefitSlots + threadIdx.x];
    tot[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (mode == 0) {
        const bool stop = tot[0] < 3.0;
        state[kStateStop] = stop ? 1.0 : 0.0;
        for (int k = 0; k < 6; ++k) state[kStateCentre + k] = stop ? 0.0 : tot[2 + k] / tot[0];
    } else if (mode == 1) {
        if (state[kStateStop] != 0.0) return;
        double hm[3][3], pm[3], qm[3], pose[12];
        for (int a = 0; a < 3; ++a) {
            pm[a] = state[kStateCentre + a];
            qm[a] = state[kStateCentre + 3 + a];
            for (int b = 0; b < 3; ++b) hm[a][b] = tot[2 + 3 * a + b];
        }
        kabsch_pose(hm, pm, qm, pose);
        for (int k = 0; k < 12; ++k) state[kStatePose + k] = pose[k];
    } else {
        state[kStateCount] = tot[0];
        state[kStateSum] = tot[1];
    }
}

__global__ __launch_bounds__(kBlock) void k_pack_pq(const double* __restrict__ p, const double* __restrict__ q, int64_t C,
                                                    double* __restrict__ pq) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        pq[c * kPq + a] = p[c * 3 + a];
        pq[c * kPq + 3 + a] = q[c * 3 + a];
    }
    pq[c * kPq + 6] = 0.0;
    pq[c * kPq + 7] = 0.0;
}

}  // namespace

struct prg_ransac {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t C = 0, H = 0;
    bool have_triples = false, have_scores = false;
    prg::DevBuf<double> pq;          // [C][kPq]
    prg::DevBuf<double> pose;        // [H][12]
    prg::DevBuf<int> valid, tri;     // [H], [H][3]
    prg::DevBuf<int> counts, part_count;
    prg::DevBuf<double> sums, part_sum;
    prg::DevBuf<double> refit_part, state, best_d;
    prg::DevBuf<int> inl, best_i;
    prg::DevBuf<int> tile_count, tile_start;
    prg::DevBuf<int> list, n_valid_dev;  // the valid hypotheses in ascending order, and how many
    int64_t n_valid = 0;
};

extern "C" {

int prg_feature_match(int device, void* hip_stream, const double* a_hd, int64_t na, const double* b_hd, int64_t nb, int d,
                      int segments, int* idx_out_hd, double* d2_out_hd) {
    return match_impl("prg_feature_match", device, hip_stream, a_hd, na, b_hd, nb, d, segments, idx_out_hd, d2_out_hd, nullptr);
}

int prg_feature_match_mutual(int device, void* hip_stream, const double* a_hd, int64_t na, const double* b_hd, int64_t nb, int d,
                             int segments, int* idx_out_hd, double* d2_out_hd, int* mutual_out_hd) {
    PRG_REQUIRE(mutual_out_hd != nullptr, PRG_ERR_INVALID, "prg_feature_match_mutual: NULL argument");
    return match_impl("prg_feature_match_mutual", device, hip_stream, a_hd, na, b_hd, nb, d, segments, idx_out_hd, d2_out_hd,
                      mutual_out_hd);
}

int prg_ransac_create(prg_ransac** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_ransac_destroy(prg_ransac* h) {
    return prg::destroy_handle(h);
}

int prg_ransac_set_correspondences(prg_ransac* h, const double* p_hd, const double* q_hd, int64_t C) {
    PRG_REQUIRE(h && p_hd && q_hd, PRG_ERR_INVALID, "prg_ransac_set_correspondences: NULL argument");
    PRG_REQUIRE(C >= 3 && C < (int64_t)1 << 31, PRG_ERR_INVALID,
                "prg_ransac_set_correspondences: need 3 <= C < 2^31 correspondences, got %lld", (long long)C);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    PRG_HIP(hipStreamSynchronize(st));
    h->C = 0;
    h->have_scores = false;
    prg::DevBuf<double> raw;
    PRG_HIP(raw.reset(C * 6));
    PRG_HIP(h->pq.ensure(C * kPq, C * kPq));
    PRG_HIP(h->inl.ensure(C, C));
    const int64_t nruns = prg::ceil_div(C, kRefitRun);
    PRG_HIP(h->refit_part.ensure(nruns * kRefitSlots, nruns * kRefitSlots));
    PRG_HIP(h->state.ensure(kStateLen, kStateLen));
    PRG_HIP(hipMemcpyAsync(raw.p, p_hd, (size_t)C * 3 * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(raw.p + C * 3, q_hd, (size_t)C * 3 * sizeof(double), hipMemcpyDefault, st));
    k_pack_pq<<<(unsigned)prg::ceil_div(C, kBlock), kBlock, 0, st>>>(raw.p, raw.p + C * 3, C, h->pq.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(st));
    h->C = C;
    return PRG_OK;
}

static int ensure_hypotheses(prg_ransac* h, int64_t H) {
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->H = 0;
    h->have_triples = h->have_scores = false;
    PRG_HIP(h->pose.ensure(H * 12, H * 12));
    PRG_HIP(h->valid.ensure(H, H));
    PRG_HIP(h->tri.ensure(H * 3, H * 3));
    PRG_HIP(h->counts.ensure(H, H));
    PRG_HIP(h->sums.ensure(H, H));
    PRG_HIP(h->list.ensure(H, H));
    PRG_HIP(h->n_valid_dev.ensure(1, 1));
    PRG_HIP(h->tile_count.ensure(prg::ceil_div(H, kCompactTile), prg::ceil_div(H, kCompactTile)));
    PRG_HIP(h->tile_start.ensure(prg::ceil_div(H, kCompactTile), prg::ceil_div(H, kCompactTile)));
    return PRG_OK;
}

int prg_ransac_build(prg_ransac* h, uint64_t seed, uint64_t h_offset, int64_t H, double edge_similarity) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ransac_build: NULL argument");
    PRG_REQUIRE(H >= 1 && H <= kMaxHyp, PRG_ERR_INVALID, "prg_ransac_build: need 1 <= H <= %lld hypotheses, got %lld",
                (long long)kMaxHyp, (long long)H);
    PRG_REQUIRE(edge_similarity >= 0.0 && edge_similarity <= 1.0, PRG_ERR_INVALID,
                "prg_ransac_build: edge_similarity must lie in [0, 1], got %g", edge_similarity);
    PRG_REQUIRE(h->C >= 3, PRG_ERR_STATE, "prg_ransac_build: no correspondences (prg_ransac_set_correspondences first)");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_hypotheses(h, H));
    k_hyp_build<<<(unsigned)prg::ceil_div(H, kBlock), kBlock, 0, h->stream>>>(h->pq.p, (uint32_t)h->C, seed, h_offset, H,
                                                                             edge_similarity, h->tri.p, h->pose.p, h->valid.p);
    PRG_HIP(hipGetLastError());
    h->H = H;
    h->have_triples = true;
    return PRG_OK;
}

int prg_ransac_get_hypotheses(prg_ransac* h, int* triples_host, double* pose_host, int* valid_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ransac_get_hypotheses: NULL argument");
    PRG_REQUIRE(h->H >= 1, PRG_ERR_STATE, "prg_ransac_get_hypotheses: prg_ransac_build or prg_ransac_set_hypotheses first");
    PRG_REQUIRE(!triples_host || h->have_triples, PRG_ERR_STATE,
                "prg_ransac_get_hypotheses: hypotheses installed by prg_ransac_set_hypotheses carry no triples");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(triples_host, h->tri, h->H * 3, h->stream));
    PRG_TRY(prg::copy_out(pose_host, h->pose, h->H * 12, h->stream));
    PRG_TRY(prg::copy_out(valid_host, h->valid, h->H, h->stream));
    return PRG_OK;
}

int prg_ransac_set_hypotheses(prg_ransac* h, const double* pose_host, const int* valid_host, int64_t H) {
    PRG_REQUIRE(h && pose_host && valid_host, PRG_ERR_INVALID, "prg_ransac_set_hypotheses: NULL argument");
    PRG_REQUIRE(H >= 1 && H <= kMaxHyp, PRG_ERR_INVALID, "prg_ransac_set_hypotheses: need 1 <= H <= %lld hypotheses, got %lld",
                (long long)kMaxHyp, (long long)H);
    PRG_ENTER(h->device);
    PRG_TRY(ensure_hypotheses(h, H));
    PRG_TRY(prg::copy_in(h->pose, pose_host, H * 12, h->stream));
    PRG_TRY(prg::copy_in(h->valid, valid_host, H, h->stream));
    h->H = H;
    return PRG_OK;
}

int prg_ransac_score(prg_ransac* h, double tau) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ransac_score: NULL argument");
    PRG_REQUIRE(std::isfinite(tau) && tau >= 0.0, PRG_ERR_INVALID, "prg_ransac_score: tau must be finite and >= 0, got %g", tau);
    PRG_REQUIRE(h->C >= 3, PRG_ERR_STATE, "prg_ransac_score: no correspondences (prg_ransac_set_correspondences first)");
    PRG_REQUIRE(h->H >= 1, PRG_ERR_STATE, "prg_ransac_score: no hypotheses (prg_ransac_build or prg_ransac_set_hypotheses first)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    const int nseg = (int)prg::ceil_div(h->C, kScoreSegment);
    const int ntiles = (int)prg::ceil_div(h->H, kCompactTile);
    k_valid_count<<<ntiles, kBlock, 0, st>>>(h->valid.p, h->H, h->tile_count.p);
    k_tile_scan<<<1, kBestThreads, 0, st>>>(h->tile_count.p, ntiles, h->tile_start.p, h->n_valid_dev.p);
    k_valid_write<<<ntiles, kBlock, 0, st>>>(h->valid.p, h->H, h->tile_start.p, h->list.p);
    k_score_fill<<<(unsigned)prg::ceil_div(h->H, kBlock), kBlock, 0, st>>>(h->H, h->counts.p, h->sums.p);
    PRG_HIP(hipGetLastError());
    int n_valid = 0;
    PRG_HIP(hipMemcpyAsync(&n_valid, h->n_valid_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    h->n_valid = n_valid;
    const int64_t batch = std::min<int64_t>(h->n_valid, kScoreBatch);
    PRG_HIP(h->part_count.ensure(nseg * batch, nseg * batch));
    PRG_HIP(h->part_sum.ensure(nseg * batch, nseg * batch));
    for (int64_t l0 = 0; l0 < h->n_valid; l0 += batch) {
        const int64_t n_l = std::min<int64_t>(batch, h->n_valid - l0);
        const dim3 grid((unsigned)prg::ceil_div(n_l, kBlock), (unsigned)nseg);
        k_hyp_score<<<grid, kBlock, 0, st>>>(h->pq.p, h->C, h->pose.p, h->list.p + l0, n_l, tau * tau, h->part_count.p,
                                             h->part_sum.p);
        k_score_merge<<<grid.x, kBlock, 0, st>>>(h->part_count.p, h->part_sum.p, nseg, h->list.p + l0, n_l, h->counts.p,
                                                 h->sums.p);
    }
    PRG_HIP(hipGetLastError());
    h->have_scores = true;
    return PRG_OK;
}

int prg_ransac_get_scores(prg_ransac* h, int* counts_host, double* sums_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ransac_get_scores: NULL argument");
    PRG_REQUIRE(h->have_scores, PRG_ERR_STATE, "prg_ransac_get_scores: prg_ransac_score first");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(counts_host, h->counts, h->H, h->stream));
    PRG_TRY(prg::copy_out(sums_host, h->sums, h->H, h->stream));
    return PRG_OK;
}

int prg_ransac_best(prg_ransac* h, int64_t* index_host, int* count_host, double* sum_host, double* pose_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ransac_best: NULL argument");
    PRG_REQUIRE(h->have_scores, PRG_ERR_STATE, "prg_ransac_best: prg_ransac_score first");
    PRG_ENTER(h->device);
    PRG_REQUIRE(h->n_valid >= 1, PRG_ERR_STATE,
                "prg_ransac_best: none of the %lld hypotheses is valid (repeated index, edge lengths or degenerate triangle)",
                (long long)h->H);
    PRG_HIP(h->best_i.ensure(2, 2));
    PRG_HIP(h->best_d.ensure(13, 13));
    k_best<<<1, kBestThreads, 0, h->stream>>>(h->counts.p, h->sums.p, h->pose.p, h->list.p, h->n_valid, h->best_i.p, h->best_d.p);
    PRG_HIP(hipGetLastError());
    int bi[2];
    double bd[13];
    PRG_HIP(hipMemcpyAsync(bi, h->best_i.p, sizeof(bi), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipMemcpyAsync(bd, h->best_d.p, sizeof(bd), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_REQUIRE(bi[0] >= 0, PRG_ERR_STATE, "prg_ransac_best: no hypothesis has a score");
    if (index_host) *index_host = bi[0];
    if (count_host) *count_host = bi[1];
    if (sum_host) *sum_host = bd[0];
    if (pose_host)
        for (int k = 0; k < 12; ++k) pose_host[k] = bd[1 + k];
    return PRG_OK;
}

int prg_ransac_refine(prg_ransac* h, double tau, int iters, double* pose_io_host, int* count_host, double* sum_host,
                      int* inlier_host) {
    PRG_REQUIRE(h && pose_io_host, PRG_ERR_INVALID, "prg_ransac_refine: NULL argument");
    PRG_REQUIRE(std::isfinite(tau) && tau >= 0.0, PRG_ERR_INVALID, "prg_ransac_refine: tau must be finite and >= 0, got %g", tau);
    PRG_REQUIRE(iters >= 0 && iters <= 1000, PRG_ERR_INVALID, "prg_ransac_refine: iters must lie in 0 .. 1000, got %d", iters);
    for (int k = 0; k < 12; ++k)
        PRG_REQUIRE(std::isfinite(pose_io_host[k]), PRG_ERR_INVALID, "prg_ransac_refine: the pose contains NaN or infinity");
    PRG_REQUIRE(h->C >= 3, PRG_ERR_STATE, "prg_ransac_refine: no correspondences (prg_ransac_set_correspondences first)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    double state[kStateLen] = {0.0};
    for (int k = 0; k < 12; ++k) state[kStatePose + k] = pose_io_host[k];
    PRG_HIP(hipMemcpyAsync(h->state.p, state, sizeof(state), hipMemcpyHostToDevice, st));
    const int64_t nruns = prg::ceil_div(h->C, kRefitRun);
    const unsigned nb = (unsigned)prg::ceil_div(nruns, kBlock);
    const double tau2 = tau * tau;
    for (int it = 0; it < iters; ++it) {
        for (int mode = 0; mode < 2; ++mode) {
            k_refit_sums<<<nb, kBlock, 0, st>>>(h->pq.p, h->C, h->state.p, tau2, mode, h->refit_part.p, nullptr);
            k_refit_step<<<1, kRefitSlots, 0, st>>>(h->refit_part.p, nruns, mode, h->state.p);
        }
    }
    k_refit_sums<<<nb, kBlock, 0, st>>>(h->pq.p, h->C, h->state.p, tau2, 0, h->refit_part.p, h->inl.p);
    k_refit_step<<<1, kRefitSlots, 0, st>>>(h->refit_part.p, nruns, 2, h->state.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(state, h->state.p, sizeof(state), hipMemcpyDeviceToHost, st));
    if (inlier_host) PRG_HIP(hipMemcpyAsync(inlier_host, h->inl.p, (size_t)h->C * sizeof(int), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < 12; ++k) pose_io_host[k] = state[kStatePose + k];
    if (count_host) *count_host = (int)state[kStateCount];
    if (sum_host) *sum_host = state[kStateSum];
    return PRG_OK;
}

}  // extern "C"
