// CPD correspondences: for every owned point the k streamed points with the largest log-domain posterior
//   s = owned_bias + streamed_bias - kappa |owned - streamed|^2        (= log2 P_mn on a plan: b_n - kappa (d^2 + q_m))
// in descending order; equal float32 scores rank by the smaller index in the CALLER's point order.  The M x N matrix P of
// cpd.py:84 is never formed: one sweep "owned points x streamed points" on the vector pipe keeps the best k per lane in
// registers, a second small kernel merges the per-segment lists.  No exponential per pair, no atomics: (score, caller index)
// is a strict total order, so the k best of a point are the same set in the same order however the streamed cloud is cut.
//
//   prg_topk_sweep                 the stage on explicit clouds and biases (zero biases: an exact k-nearest-neighbour search)
//   prg_cpd_correspond             ... on a plan after prg_cpd_estep: z4 (q_m in .w), tgt4 (b_n in .w), perm_src / perm_tgt
//   prg_cpd_correspond_tile_shape  the sweep's tile (tests place sizes at its edges)
#include <algorithm>
#include <cmath>

#include "cpd_plan.h"
#include "dev_buf.h"

namespace {

constexpr int kOwned = 256;   // owned points per workgroup: one per lane
constexpr int kTile = 8;      // streamed points per trip of the sweep's loop (wave-uniform addresses: scalar loads)
constexpr int kMaxK = 8;
constexpr int kMaxSegments = 4096;
constexpr double kLog2e = 1.4426950408889634;

// (v, j) ranks ahead of the list entry (s, id): the larger score, or the same score and the smaller index in the caller's
// order (perm: kernel order -> caller's order; null: they are the same).  An empty slot (id < 0) loses to every candidate; a
// NaN score is ahead of nothing.  The index loads happen on the equal path only.
__device__ __forceinline__ bool ranks_ahead(float v, int j, float s, int id, const int* __restrict__ perm) {
    if (v != s) return v > s;
    if (id < 0) return true;
    return perm ? perm[j] < perm[id] : j < id;
}

// Compare-and-shift insertion into a descending list of K registers; every index is a compile-time constant.
template <int K>
__device__ __forceinline__ void list_insert(float (&s)[K], int (&id)[K], float v, int j, const int* __restrict__ perm) {
    bool a[K];
#pragma unroll
    for (int r = 0; r < K; ++r) a[r] = ranks_ahead(v, j, s[r], id[r], perm);
#pragma unroll
    for (int r = K - 1; r > 0; --r) {
        s[r] = a[r - 1] ? s[r - 1] : (a[r] ? v : s[r]);
        id[r] = a[r - 1] ? id[r - 1] : (a[r] ? j : id[r]);
    }
    s[0] = a[0] ? v : s[0];
    id[0] = a[0] ? j : id[0];
}

// Lane i owns point i; the workgroup streams segment blockIdx.y = [y seg_len, min((y + 1) seg_len, n_s)) of the streamed
// cloud.  Nothing past the real count n_s is ever read, so no pad can enter a list.  The list carries kernel-order indices.
// part_s / part_id: [segment][K][n_o].
template <int K>
__global__ __launch_bounds__(kOwned) void k_topk_sweep(const float4* __restrict__ own4, int64_t n_o,
                                                       const float4* __restrict__ str4, int64_t n_s, int64_t seg_len,
                                                       float neg_kappa, const int* __restrict__ perm_s,
                                                       float* __restrict__ part_s, int* __restrict__ part_id) {
    const int64_t i_own = (int64_t)blockIdx.x * kOwned + threadIdx.x;
    const float4 a = own4[i_own < n_o ? i_own : n_o - 1];  // lanes past the end redo the last point and store nothing
    const int64_t j0 = (int64_t)blockIdx.y * seg_len;
    const int64_t j1 = j0 + seg_len < n_s ? j0 + seg_len : n_s;
    float s[K];
    int id[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        s[r] = -INFINITY;
        id[r] = -1;
    }
    auto visit = [&](const float4 q, int j) {
        const float dx = __fsub_rn(a.x, q.x), dy = __fsub_rn(a.y, q.y), dz = __fsub_rn(a.z, q.z);
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, __fmul_rn(dx, dx)));
        const float v = __fadd_rn(a.w, fmaf(neg_kappa, d2, q.w));
        if (v >= s[K - 1]) list_insert<K>(s, id, v, j, perm_s);
    };
    int64_t j = j0;
    for (; j + kTile <= j1; j += kTile) {
        float4 q[kTile];  // the whole tile is requested before the first point is looked at: one wait per tile
#pragma unroll
        for (int c = 0; c < kTile; ++c) q[c] = str4[j + c];
#pragma unroll
        for (int c = 0; c < kTile; ++c) visit(q[c], (int)(j + c));
    }
    for (; j < j1; ++j) visit(str4[j], (int)j);
    if (i_own < n_o) {
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const int64_t o = ((int64_t)blockIdx.y * K + r) * n_o + i_own;
            part_s[o] = s[r];
            part_id[o] = id[r];
        }
    }
}

// The segments' lists of one owned point -> its list, with the sweep's comparator; rows and entries leave in the caller's
// order (perm_o / perm_s: kernel order -> caller's order, null: the same), cut back to the k_out the caller asked for;
// prob_out (may be null): exp2 of the score in fp64.
template <int K>
__global__ __launch_bounds__(kOwned) void k_topk_merge(const float* __restrict__ part_s, const int* __restrict__ part_id,
                                                       int nseg, int64_t n_o, const int* __restrict__ perm_s,
                                                       const int* __restrict__ perm_o, int k_out,
                                                       int* __restrict__ index_out, float* __restrict__ score_out,
                                                       double* __restrict__ prob_out) {
    const int64_t i = (int64_t)blockIdx.x * kOwned + threadIdx.x;
    if (i >= n_o) return;
    float s[K];
    int id[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        s[r] = part_s[(int64_t)r * n_o + i];
        id[r] = part_id[(int64_t)r * n_o + i];
    }
    for (int g = 1; g < nseg; ++g) {
        float v[K];
        int j[K];
#pragma unroll
        for (int r = 0; r < K; ++r) {
            v[r] = part_s[((int64_t)g * K + r) * n_o + i];
            j[r] = part_id[((int64_t)g * K + r) * n_o + i];
        }
#pragma unroll
        for (int r = 0; r < K; ++r)
            if (j[r] >= 0 && v[r] >= s[K - 1]) list_insert<K>(s, id, v[r], j[r], perm_s);
    }
    const int64_t row = perm_o ? perm_o[i] : i;
#pragma unroll
    for (int r = 0; r < K; ++r) {
        if (r < k_out) {
            index_out[row * k_out + r] = id[r] < 0 ? -1 : (perm_s ? perm_s[id[r]] : id[r]);
            score_out[row * k_out + r] = s[r];
            // (on the device: a probability in fp64's subnormal range costs the host's libm 75 ns apiece)
            if (prob_out) prob_out[row * k_out + r] = exp2((double)s[r]);
        }
    }
}

// explicit cloud [n][dim] + optional bias [n] -> (x, y, z, bias)
__global__ __launch_bounds__(kOwned) void k_corr_pack(const float* __restrict__ pts, const float* __restrict__ bias,
                                                      int64_t n, int dim, float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kOwned + threadIdx.x;
    if (i >= n) return;
    out[i] = make_float4(pts[i * dim], pts[i * dim + 1], dim > 2 ? pts[i * dim + 2] : 0.f, bias ? bias[i] : 0.f);
}

// A plan's cloud as the sweep takes it.  SOURCE: z4, bias = -kappa q_m = log2 a_m.  Otherwise tgt4, bias = b_n; a column
// whose denominator underflowed carries b_n = -inf after the E-step (its column of P is zero) and gets the bias of the
// definition here: den = float32 eps (cpd.py:81), then + c.
template <bool SOURCE>
__global__ __launch_bounds__(kOwned) void k_corr_pack_plan(const float4* __restrict__ in, int64_t n, float neg_kappa,
                                                           float dead_bias, float4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kOwned + threadIdx.x;
    if (i >= n) return;
    float4 p = in[i];
    if (SOURCE)
        p.w = __fmul_rn(neg_kappa, p.w);
    else if (p.w == -INFINITY)
        p.w = dead_bias;
    out[i] = p;
}

int template_k(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

// segments of the streamed cloud: (count, length).  Automatic: enough (block, segment) workgroups to fill the chip even for
// a few thousand owned points, as prg_nn_mean_distance cuts its sweep.
void cut_segments(int64_t n_o, int64_t n_s, int segments, int* nseg, int64_t* seg_len) {
    int64_t want = segments;
    if (want <= 0) {
        const int64_t nbx = prg::ceil_div(n_o, kOwned);
        want = std::min<int64_t>(std::max<int64_t>(1, 2048 / nbx), prg::ceil_div(n_s, 256));
    }
    want = std::min<int64_t>(want, n_s);
    *seg_len = prg::ceil_div(n_s, want);
    *nseg = (int)prg::ceil_div(n_s, *seg_len);  // no empty segment
}

// How one call cuts the streamed cloud, and what its partial lists take: [nseg][kt][n_o] scores and as many indices
struct TopkCut {
    int nseg, kt;
    int64_t seg_len, part_elems;
};
TopkCut cut_topk(int64_t n_o, int64_t n_s, int k, int segments) {
    TopkCut c;
    cut_segments(n_o, n_s, segments, &c.nseg, &c.seg_len);
    c.kt = template_k(k);
    c.part_elems = (int64_t)c.nseg * c.kt * n_o;
    return c;
}

// own4 [n_o], str4 [n_s] on the device -> idx_dev / score_dev [n_o][k] on the device, in the caller's order; part_s / part_id:
// c.part_elems each, the caller's.  Enqueues only.
int run_topk(hipStream_t st, const float4* own4, int64_t n_o, const float4* str4, int64_t n_s, float kappa, int k,
             const TopkCut& c, const int* perm_o, const int* perm_s, float* part_s, int* part_id, int* idx_dev,
             float* score_dev, double* prob_dev) {
    const dim3 grid((unsigned)prg::ceil_div(n_o, kOwned), (unsigned)c.nseg);
    const unsigned gm = (unsigned)prg::ceil_div(n_o, kOwned);
#define PRG_TOPK_LAUNCH(K)                                                                                              \
    k_topk_sweep<K><<<grid, kOwned, 0, st>>>(own4, n_o, str4, n_s, c.seg_len, -kappa, perm_s, part_s, part_id);         \
    k_topk_merge<K><<<gm, kOwned, 0, st>>>(part_s, part_id, c.nseg, n_o, perm_s, perm_o, k, idx_dev, score_dev, prob_dev)
    switch (c.kt) {
        case 1: PRG_TOPK_LAUNCH(1); break;
        case 2: PRG_TOPK_LAUNCH(2); break;
        case 4: PRG_TOPK_LAUNCH(4); break;
        default: PRG_TOPK_LAUNCH(8); break;
    }
#undef PRG_TOPK_LAUNCH
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_cpd_correspond_tile_shape(int* owned_per_workgroup, int* streamed_per_tile) {
    PRG_REQUIRE(owned_per_workgroup && streamed_per_tile, PRG_ERR_INVALID, "prg_cpd_correspond_tile_shape: NULL argument");
    *owned_per_workgroup = kOwned;
    *streamed_per_tile = kTile;
    return PRG_OK;
}

int prg_topk_sweep(int device, void* hip_stream, const float* owned_hd, const float* owned_bias_hd, const float* streamed_hd,
                   const float* streamed_bias_hd, int64_t n_o, int64_t n_s, int dim, double kappa, int k, int segments,
                   int* index_out_hd, float* score_out_hd) {
    PRG_REQUIRE(owned_hd && streamed_hd && index_out_hd && score_out_hd, PRG_ERR_INVALID, "prg_topk_sweep: NULL argument");
    PRG_REQUIRE(n_o > 0 && n_s > 0 && n_o < (int64_t)1 << 31 && n_s < (int64_t)1 << 31 && (dim == 2 || dim == 3),
                PRG_ERR_INVALID, "prg_topk_sweep: need 0 < n_o, n_s < 2^31 and dim in {2,3}");
    PRG_REQUIRE(k >= 1 && k <= kMaxK && k <= n_s, PRG_ERR_INVALID,
                "prg_topk_sweep: k must be in [1, %d] and at most the %lld streamed points (got %d)", kMaxK, (long long)n_s, k);
    PRG_REQUIRE(std::isfinite(kappa) && kappa >= 0.0, PRG_ERR_INVALID, "prg_topk_sweep: kappa must be finite and >= 0");
    PRG_REQUIRE(segments >= 0 && segments <= kMaxSegments, PRG_ERR_INVALID, "prg_topk_sweep: segments must be in [0, %d]",
                kMaxSegments);
    PRG_ENTER(device);
    hipStream_t st = (hipStream_t)hip_stream;
    const TopkCut cut = cut_topk(n_o, n_s, k, segments);
    prg::DevBuf<float> raw_o, raw_s, bs, ps;
    prg::DevBuf<float4> o4, s4;
    prg::DevBuf<int> bi, pi;
    PRG_HIP(ps.reset(cut.part_elems));
    PRG_HIP(pi.reset(cut.part_elems));
    // one staging block per cloud: [n][dim] points, then [n] biases
    PRG_HIP(raw_o.reset(n_o * (dim + 1)));
    PRG_HIP(raw_s.reset(n_s * (dim + 1)));
    PRG_HIP(o4.reset(n_o));
    PRG_HIP(s4.reset(n_s));
    PRG_HIP(bi.reset(n_o * k));
    PRG_HIP(bs.reset(n_o * k));
    float* const ob = raw_o.p + n_o * dim;
    float* const sb = raw_s.p + n_s * dim;
    PRG_HIP(hipMemcpyAsync(raw_o.p, owned_hd, (size_t)n_o * dim * sizeof(float), hipMemcpyDefault, st));
    if (owned_bias_hd) PRG_HIP(hipMemcpyAsync(ob, owned_bias_hd, (size_t)n_o * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(raw_s.p, streamed_hd, (size_t)n_s * dim * sizeof(float), hipMemcpyDefault, st));
    if (streamed_bias_hd) PRG_HIP(hipMemcpyAsync(sb, streamed_bias_hd, (size_t)n_s * sizeof(float), hipMemcpyDefault, st));
    k_corr_pack<<<(unsigned)prg::ceil_div(n_o, kOwned), kOwned, 0, st>>>(raw_o.p, owned_bias_hd ? ob : nullptr, n_o, dim, o4.p);
    k_corr_pack<<<(unsigned)prg::ceil_div(n_s, kOwned), kOwned, 0, st>>>(raw_s.p, streamed_bias_hd ? sb : nullptr, n_s, dim, s4.p);
    PRG_HIP(hipGetLastError());
    PRG_TRY(run_topk(st, o4.p, n_o, s4.p, n_s, (float)kappa, k, cut, nullptr, nullptr, ps.p, pi.p, bi.p, bs.p, nullptr));
    PRG_HIP(hipMemcpyAsync(index_out_hd, bi.p, (size_t)n_o * k * sizeof(int), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(score_out_hd, bs.p, (size_t)n_o * k * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

int prg_cpd_correspond(prg_cpd* h, int side, int k, int* index_out, float* log2_prob_out, double* prob_out) {
    PRG_REQUIRE(h && index_out, PRG_ERR_INVALID, "prg_cpd_correspond: NULL argument");
    PRG_REQUIRE(side == 0 || side == 1, PRG_ERR_INVALID, "prg_cpd_correspond: side must be 0 (source) or 1 (target)");
    PRG_REQUIRE(h->have_source && h->have_target && h->have_estep, PRG_ERR_STATE, "prg_cpd_correspond: no E-step has been run");
    PRG_REQUIRE(h->estep_state_live, PRG_ERR_STATE,
                "prg_cpd_correspond: the plan has moved on since its last prg_cpd_estep (an M-step, new parameters, new weights or "
                "prg_cpd_moments_from_estep): tgt4.w no longer holds the b_n of the sigma2 in PARAMS - run prg_cpd_estep first");
    PRG_REQUIRE(h->Nglobal == h->N, PRG_ERR_STATE,
                "prg_cpd_correspond: the target is sharded over ranks (%lld of %lld points here): not supported",
                (long long)h->N, (long long)h->Nglobal);
    const int64_t n_o = side == 0 ? h->M : h->N, n_s = side == 0 ? h->N : h->M;
    PRG_REQUIRE(k >= 1 && k <= kMaxK && k <= n_s, PRG_ERR_INVALID,
                "prg_cpd_correspond: k must be in [1, %d] and at most the %lld streamed points (got %d)", kMaxK, (long long)n_s, k);
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    double sigma2 = 0.0;
    PRG_HIP(hipMemcpyAsync(&sigma2, h->params + 13, sizeof(double), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    PRG_REQUIRE(sigma2 > 0.0 && std::isfinite(sigma2), PRG_ERR_STATE, "prg_cpd_correspond: sigma2 = %g", sigma2);
    // kappa and the outlier constant exactly as the E-step's merge kernels form them (k_colfinal)
    const float kappa = -(float)(-kLog2e / (2.0 * sigma2));
    const double w = h->last_w;
    const double ratio = h->uniform_ratio > 0.0 ? h->uniform_ratio : (double)h->M / (double)h->Nglobal;
    const double c = w > 0.0 ? std::pow(2.0 * M_PI * sigma2, h->D * 0.5) * (w / (1.0 - w) * ratio) : 0.0;
    const float dead_bias = (float)(-std::log2(1.1920928955078125e-07 + c));
    // the workspace, carved in 256-byte steps: packed source, packed target, results (index, score), partial lists (score, index),
    // probabilities
    const TopkCut cut = cut_topk(n_o, n_s, k, 0);
    const size_t sizes[7] = {(size_t)h->M * sizeof(float4), (size_t)h->N * sizeof(float4), (size_t)n_o * k * sizeof(int),
                             (size_t)n_o * k * sizeof(float), (size_t)cut.part_elems * sizeof(float),
                             (size_t)cut.part_elems * sizeof(int), (size_t)n_o * k * sizeof(double)};
    size_t off[8] = {0};
    for (int i = 0; i < 7; ++i) off[i + 1] = off[i] + (size_t)prg::round_up((int64_t)sizes[i], 256);
    // ... one block that grows and is never shrunk, so that a call on a plan allocates nothing once it has run at its largest k:
    // a free drains the device and a fresh 16 MB allocation costs more than the sweep
    if (h->corr_buf.cap < (int64_t)off[7]) PRG_HIP(hipStreamSynchronize(st));
    PRG_HIP(h->corr_buf.ensure((int64_t)off[7], (int64_t)off[7]));
    char* const base = h->corr_buf.p;
    float4* const z4 = reinterpret_cast<float4*>(base + off[0]);
    float4* const x4 = reinterpret_cast<float4*>(base + off[1]);
    int* const bi = reinterpret_cast<int*>(base + off[2]);
    float* const bs = reinterpret_cast<float*>(base + off[3]);
    float* const ps = reinterpret_cast<float*>(base + off[4]);
    int* const pi = reinterpret_cast<int*>(base + off[5]);
    double* const bp = reinterpret_cast<double*>(base + off[6]);
    k_corr_pack_plan<true><<<(unsigned)prg::ceil_div(h->M, kOwned), kOwned, 0, st>>>(h->z4.p, h->M, -kappa, 0.f, z4);
    k_corr_pack_plan<false><<<(unsigned)prg::ceil_div(h->N, kOwned), kOwned, 0, st>>>(h->tgt4.p, h->N, 0.f, dead_bias, x4);
    PRG_HIP(hipGetLastError());
    const float4* const own4 = side == 0 ? z4 : x4;
    const float4* const str4 = side == 0 ? x4 : z4;
    PRG_TRY(run_topk(st, own4, n_o, str4, n_s, kappa, k, cut, side == 0 ? h->perm_src.p : h->perm_tgt.p,
                     side == 0 ? h->perm_tgt.p : h->perm_src.p, ps, pi, bi, bs, prob_out ? bp : nullptr));
    PRG_HIP(hipMemcpyAsync(index_out, bi, (size_t)n_o * k * sizeof(int), hipMemcpyDeviceToHost, st));
    if (log2_prob_out) PRG_HIP(hipMemcpyAsync(log2_prob_out, bs, (size_t)n_o * k * sizeof(float), hipMemcpyDeviceToHost, st));
    if (prob_out) PRG_HIP(hipMemcpyAsync(prob_out, bp, (size_t)n_o * k * sizeof(double), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

}  // extern "C"
