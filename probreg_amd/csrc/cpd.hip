// The CPD plan for MI355X (gfx950): lifecycle, cloud uploads, the device M-step and the C ABI of the CPD EM iteration.
// The E-step - its layout, the engine decision, the launches and the merge / moment kernels - lives in cpd_estep.hip, the pair
// sweeps in cpd_sweeps_*.hip.
//
// Reference behaviour (neka-nat/probreg v0.3.7):
//   E-step   probreg/cpd.py:71-88          M-step rigid  probreg/cpd.py:160-192
//   M-step affine probreg/cpd.py:219-244   transforms    probreg/transformation.py:49-50, 77-78
//   k_mstep    one thread, fp64: 3x3 one-sided Jacobi SVD / 3x3 solve, sigma2, q.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cpd_estep.h"
#include "cpd_mstep.h"
#include "cpd_sweeps.h"
#include "morton.h"
#include "small_linalg.h"

namespace {
using prg::block_reduce_store;
using prg::ensure_mompart;
using prg::grid1;
using prg::kBlock;
using prg::kMomComp;
using prg::row_moment_terms;


// ---------------------------------------------------------------------------------------------
// layout / upload helpers
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_pack_cloud(const float* __restrict__ in, int64_t n, int dim,
                                                       float4* __restrict__ out, int64_t cap, float pad,
                                                       float aux, const int* __restrict__ perm) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= cap) return;
    float4 v;
    if (i < n) {
        const int64_t j = perm ? perm[i] : i;  // sorted position i holds original point perm[i]
        v.x = in[j * dim];
        v.y = in[j * dim + 1];
        v.z = dim > 2 ? in[j * dim + 2] : 0.f;
        v.w = aux;
    } else {
        v.x = v.y = v.z = pad;
        v.w = 0.f;
    }
    out[i] = v;
}

// sum of coordinates and of squared norms: partials [nblk][4]
__global__ __launch_bounds__(kBlock) void k_cloud_sums(const float4* __restrict__ pts, int64_t n,
                                                       double* __restrict__ part) {
    __shared__ double sh[4][4];
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double a[4] = {0, 0, 0, 0};
    if (i < n) {
        float4 v = pts[i];
        a[0] = v.x; a[1] = v.y; a[2] = v.z;
        a[3] = (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        double s = wave_sum(a[c]);
        if (lane == 0) sh[wv][c] = s;
    }
    __syncthreads();
    if (threadIdx.x < 4) part[(int64_t)blockIdx.x * 4 + threadIdx.x] =
        sh[0][threadIdx.x] + sh[1][threadIdx.x] + sh[2][threadIdx.x] + sh[3][threadIdx.x];
}

__global__ void k_zero_doubles(double* p, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0;
}

// sigma2_0 = [M sum|x|^2 + N sum|y|^2 - 2 (sum x).(sum y)] / (D M N)   (math_utils.py:28-29 in closed form)
// q0 = 1 + N D / 2 log(sigma2_0)                                           (cpd.py:148)
__global__ void k_init_params(double* __restrict__ moments, const double* __restrict__ srcsum,
                              double* __restrict__ params, double m, double nglobal, int dim,
                              const double* __restrict__ init /* 16 doubles or null */) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double* ts = moments + 24;
    double cross = ts[0] * srcsum[0] + ts[1] * srcsum[1] + ts[2] * srcsum[2];
    double total = m * ts[3] + nglobal * srcsum[3] - 2.0 * cross;
    if (init) {
        // the caller subtracted different origins from the two clouds (delta = origin_target - origin_source):
        // sum |x' - y' + delta|^2 = sum |x' - y'|^2 + 2 delta.(M sum x' - N sum y') + M N |delta|^2
        const double* dl = init + 13;
        double lin = 0.0, d2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            lin += dl[k] * (m * ts[k] - nglobal * srcsum[k]);
            d2 += dl[k] * dl[k];
        }
        total += 2.0 * lin + m * nglobal * d2;
    }
    double sigma2 = total / (dim * m * nglobal);
    for (int i = 0; i < PRG_NPARAMS; ++i) params[i] = 0.0;
    if (init) {
        for (int i = 0; i < 13; ++i) params[i] = init[i];
    } else {
        params[0] = params[4] = params[8] = 1.0;
        params[12] = 1.0;
    }
    params[13] = sigma2;
    params[14] = 1.0 + nglobal * dim * 0.5 * log(sigma2);
    // the target sums have served their purpose: keep the all-reduced block bounded over the EM iterations
    for (int i = 24; i < PRG_NMOMENTS; ++i) moments[i] = 0.0;
}

// bounding box (+ range of .w) of every group of 32 consecutive points -> meta[g][8] = lo.xyz, hi.xyz, max w, min w
__global__ __launch_bounds__(kBlock) void k_group_meta(const float4* __restrict__ pts, int64_t ngroups,
                                                       float* __restrict__ meta) {
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= ngroups) return;
    const float4* p = pts + g * prg::kGroup;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, wmax = -INFINITY,
          wmin = INFINITY;
    // a group that holds real points AND pads (the last real group of a cloud) gets the box of its real points: a pad never
    // contributes to any sum, and a box that reaches out to the pads (1e18 away) makes its owner need every cell of the other cloud
    const bool mixed = fabsf(p[0].x) < 1e17f && !(fabsf(p[prg::kGroup - 1].x) < 1e17f);  // (pads fill the tail)
    for (int k = 0; k < prg::kGroup; ++k) {
        const float4 v = p[k];
        if (mixed && !(fabsf(v.x) < 1e17f)) continue;
        lo[0] = fminf(lo[0], v.x); hi[0] = fmaxf(hi[0], v.x);
        lo[1] = fminf(lo[1], v.y); hi[1] = fmaxf(hi[1], v.y);
        lo[2] = fminf(lo[2], v.z); hi[2] = fmaxf(hi[2], v.z);
        wmax = fmaxf(wmax, v.w);
        wmin = fminf(wmin, v.w);
    }
    float* o = meta + g * 8;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2];
    o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
    o[6] = wmax;
    o[7] = wmin;
}

// Moments from explicit EstepResult arrays (public maximization_step path, cpd.py:90-93):
// rows (p1, px) -> comps 0..21 ; columns (pt1, x) -> comp 22.  grid covers max(M, N) items.
__global__ __launch_bounds__(kBlock) void k_moments_from_arrays(const double* __restrict__ pt1,
                                                                const double* __restrict__ p1,
                                                                const double* __restrict__ px, int dim, int64_t m,
                                                                int64_t n, const float4* __restrict__ src4,
                                                                const float4* __restrict__ tgt4,
                                                                const int* __restrict__ perm_src,
                                                                const int* __restrict__ perm_tgt,
                                                                double* __restrict__ mompart) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double a[kMomComp];
#pragma unroll
    for (int c = 0; c < kMomComp; ++c) a[c] = 0.0;
    if (i < m) {
        const float4 yf = src4[i];
        const double y[3] = {yf.x, yf.y, yf.z};
        const int64_t j = perm_src ? perm_src[i] : i;  // the caller's arrays are in the original point order
        double pxi[3] = {px[j * dim], px[j * dim + 1], dim > 2 ? px[j * dim + 2] : 0.0};
        row_moment_terms(a, p1[j], pxi, y);
    }
    if (i < n) {
        const float4 xf = tgt4[i];
        const int64_t j = perm_tgt ? perm_tgt[i] : i;
        a[22] = pt1[j] * ((double)xf.x * xf.x + (double)xf.y * xf.y + (double)xf.z * xf.z);
    }
    block_reduce_store(a, mompart);
}

// The same arrays as the per-point fp64 block [4][Mcap] (p1, px) the non-rigid solve reads (kernel order).
__global__ __launch_bounds__(kBlock) void k_rowacc_from_arrays(const double* __restrict__ pt1,
                                                               const double* __restrict__ p1,
                                                               const double* __restrict__ px, int dim, int64_t m,
                                                               int64_t n, int64_t mcap,
                                                               const int* __restrict__ perm_src,
                                                               const int* __restrict__ perm_tgt,
                                                               double* __restrict__ rowacc, float* __restrict__ pt1f) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) pt1f[i] = (float)pt1[perm_tgt ? perm_tgt[i] : i];
    if (i >= m) return;
    const int64_t j = perm_src ? perm_src[i] : i;
    rowacc[i] = p1[j];
    rowacc[mcap + i] = px[j * dim];
    rowacc[2 * mcap + i] = px[j * dim + 1];
    rowacc[3 * mcap + i] = dim > 2 ? px[j * dim + 2] : 0.0;
}

// ---------------------------------------------------------------------------------------------
// device M-step (fp64, one thread)
// ---------------------------------------------------------------------------------------------
// kind: PRG_TF_RIGID (cpd.py:160-192) or PRG_TF_AFFINE (cpd.py:219-244).
__global__ void k_mstep(const double* __restrict__ mom, double* __restrict__ params, int kind, int update_scale,
                        int dim) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    prg::mstep_body(mom, params, kind, update_scale, dim);  // (cpd_mstep.h: shared with the batch plan)
}

// EstepResult materialisation helpers
// Outputs go back to the caller's point order: sorted position i holds original point perm[i].
__global__ __launch_bounds__(kBlock) void k_float_to_double(const float* __restrict__ in, double* __restrict__ out,
                                                            int64_t n, const int* __restrict__ perm) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[perm ? perm[i] : i] = in[i];
}
__global__ __launch_bounds__(kBlock) void k_scatter_double(const double* __restrict__ in, double* __restrict__ out,
                                                           int64_t n, const int* __restrict__ perm) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[perm ? perm[i] : i] = in[i];
}
// srcw[i] = (float) lw[perm[i]]  (sorted position i holds original point perm[i])
__global__ __launch_bounds__(kBlock) void k_gather_weights(const double* __restrict__ lw, int64_t m,
                                                           const int* __restrict__ perm, float* __restrict__ out) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < m) out[i] = (float)lw[perm ? perm[i] : i];
}
__global__ __launch_bounds__(kBlock) void k_pack_px(const double* __restrict__ rowacc, int64_t mcap, int64_t m,
                                                    int dim, double* __restrict__ out, const int* __restrict__ perm) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int64_t j = perm ? perm[i] : i;
    for (int k = 0; k < dim; ++k) out[j * dim + k] = rowacc[(int64_t)(1 + k) * mcap + i];
}
__global__ __launch_bounds__(kBlock) void k_unpack_points(const float4* __restrict__ in, int64_t m, int dim,
                                                          float* __restrict__ out, const int* __restrict__ perm) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const float4 v = in[i];
    const int64_t j = perm ? perm[i] : i;
    out[j * dim] = v.x;
    out[j * dim + 1] = v.y;
    if (dim > 2) out[j * dim + 2] = v.z;
}

// capacity: the cloud + room for the segments' rounding to 256-point multiples + prefetch slack
int cap_for(int64_t n) { return (int)prg::round_up(n + 64 * prg::kSuper + 1024, 1024); }

// the motion slots, allocated once and zeroed (whichever cloud is set first)
int ensure_motion(prg_cpd* h) {
    if (h->motion.p) return PRG_OK;
    PRG_HIP(h->motion.reset(16));
    PRG_HIP(hipMemsetAsync(h->motion.p, 0, 16 * sizeof(unsigned), h->stream));
    return PRG_OK;
}

// Spatial order of a cloud: sorted position -> original index, as the plan's device permutation.  [r6] The kd-tree order of
// morton.h, built on the device (spatial_order.hip: ~2 ms per 100k points; PRG_SPATIAL_ORDER=kd_host: the host build, 17 ms;
// =morton: the Z-curve of rounds 1 - 5).
int morton_permutation(prg_cpd* h, const float* pts_hd, int64_t n, int dim, prg::DevBuf<int>* perm_dev, double* ext2 = nullptr,
                       float* box = nullptr) {
    std::vector<float> host((size_t)n * dim);
    PRG_HIP(hipMemcpy(host.data(), pts_hd, host.size() * sizeof(float), hipMemcpyDefault));
    if (ext2) {  // squared diagonal of the cloud's bounding box (scale of the dense-regime criterion); box = lo.xyz, hi.xyz
        *ext2 = 0.0;
        for (int k = 0; k < 3; ++k) {
            float lo = INFINITY, hi = -INFINITY;
            for (int64_t i = 0; i < n && k < dim; ++i) {
                lo = std::min(lo, host[(size_t)i * dim + k]);
                hi = std::max(hi, host[(size_t)i * dim + k]);
            }
            if (k >= dim) lo = hi = 0.f;
            *ext2 += (double)(hi - lo) * (double)(hi - lo);
            if (box) {
                box[k] = lo;
                box[3 + k] = hi;
            }
        }
    }
    PRG_HIP(perm_dev->reset(n));
    const std::string& order = prg::cpd_env().spatial_order;
    if (order != "morton" && order != "kd_host") {
        // the caller's layout, [n][dim] floats, goes to the staging buffer (where k_pack_cloud reads it anyway) and is ordered there
        PRG_TRY(prg::ensure_stage(h, (size_t)n * dim * sizeof(float)));
        PRG_HIP(hipMemcpyAsync(h->stage.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
        return prg::device_kd_order((const float*)h->stage.p, n, dim, perm_dev->p, h->stream);
    }
    const std::vector<int> perm = order == "morton" ? prg::morton_order(host.data(), n, dim) : prg::kd_order(host.data(), n, dim);
    PRG_HIP(hipMemcpy(perm_dev->p, perm.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    return PRG_OK;
}

}  // namespace

namespace prg {
int ensure_stage(prg_cpd* h, size_t bytes) {
    if (h->stage.cap >= (int64_t)bytes) return PRG_OK;
    if (h->stage.p) PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(h->stage.reset((int64_t)bytes));
    return PRG_OK;
}

// the plan's environment knobs, read at the first use (what each one does: CpdEnv, cpd_plan.h)
const CpdEnv& cpd_env() {
    static const CpdEnv env = [] {
        CpdEnv e;
        auto num = [](const char* name, double absent) { const char* v = getenv(name); return v ? atof(v) : absent; };
        auto is_zero = [](const char* name) { const char* v = getenv(name); return v && atoi(v) == 0; };
        e.mfma_seg = getenv("PRG_MFMA_SEG") ? atoi(getenv("PRG_MFMA_SEG")) : 0;
        e.fine_grid_off = is_zero("PRG_MFMA_FINE_GRID");
        e.mfma_deal = getenv("PRG_MFMA_DEAL") ? (atoi(getenv("PRG_MFMA_DEAL")) != 0 ? 1 : 0) : -1;
        e.mfma_deal_below = num("PRG_MFMA_DEAL_BELOW", 0.9);
        e.r_col = num("PRG_ENGINE_RCOL", 0.0);
        e.r_row = num("PRG_ENGINE_RROW", 0.0);
        e.fused_rcol_scale = num("PRG_FUSED_RCOL_SCALE", -1.0);
        e.lean_factor = num("PRG_LEAN_FACTOR", -1.0);
        e.fused_factor = num("PRG_FUSED_FACTOR", -1.0);
        e.owner_off = is_zero("PRG_OWNER_SWEEP");
        e.debug_engine = getenv("PRG_DEBUG_ENGINE") != nullptr;
        if (const char* v = getenv("PRG_SPATIAL_ORDER")) e.spatial_order = v;
        return e;
    }();
    return env;
}

// Device / mapped-host state of the engine decision (EngineState, cpd_plan.h), allocated once
int ensure_engine_state(prg_cpd* h) {
    if (h->eng_dev.p) return PRG_OK;
    PRG_HIP(h->eng_host.ensure(1, kMailboxFlags));
    h->eng_host_dev = h->eng_host.dev;
    PRG_HIP(h->eng_dev.reset(1));
    PRG_HIP(hipMemsetAsync(h->eng_dev.p, 0, sizeof(EngineState), h->stream));
    h->eng_work = h->eng_dev.p->work;
    h->tsum_local = h->eng_dev.p->tsum;
    return PRG_OK;
}
}  // namespace prg

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int prg_cpd_create(prg_cpd** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream, [](prg_cpd* h) -> int {
        // defaults of a new plan from the environment (CpdEnv, cpd_plan.h: these three are read per plan, not once per process)
        if (const char* eng = getenv("PRG_DENSE_ENGINE")) h->dense_engine = std::max(0, std::min(2, atoi(eng)));
        if (const char* eng = getenv("PRG_SPARSE_ENGINE")) h->sparse_engine = std::max(0, std::min(2, atoi(eng)));
        if (const char* eng = getenv("PRG_RESID_SWEEP")) h->resid_sweep = atoi(eng) != 0;  // (A/B runs of the two-sweep sparse regime)
        PRG_HIP(h->state.reset(PRG_NMOMENTS + PRG_NPARAMS));
        h->moments = h->state.p;
        h->params = h->state.p + PRG_NMOMENTS;
        k_zero_doubles<<<1, 64, 0, h->stream>>>(h->state.p, PRG_NMOMENTS + PRG_NPARAMS);
        return PRG_OK;
    });
}

int prg_cpd_destroy(prg_cpd* h) {
    return prg::destroy_handle(h, [](prg_cpd* p) { prg::nonrigid_free(p); });  // (its buffers go with it, on the plan's device)
}

int prg_cpd_set_source(prg_cpd* h, const float* source_hd, int64_t m, int dim) {
    PRG_REQUIRE(h && source_hd, PRG_ERR_INVALID, "prg_cpd_set_source: NULL argument");
    PRG_REQUIRE(m > 0 && (dim == 2 || dim == 3), PRG_ERR_INVALID,
                "prg_cpd_set_source: need m > 0 and dim in {2,3} (got m=%lld dim=%d)", (long long)m, dim);
    PRG_REQUIRE(!h->have_target || h->D == dim, PRG_ERR_INVALID,
                "prg_cpd_set_source: dim %d does not match target dim %d", dim, h->D);
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    // no source until this one is complete: a failure below leaves a plan that says so, whatever the arrays hold by then
    h->have_source = h->have_estep = h->estep_state_live = false;
    prg::nonrigid_free(h);  // ... and nothing that belongs to the previous source: its kernel matrix, W, priors and weights
    h->srcw.release();
    h->uniform_ratio = 0.0;
    const int64_t cap = cap_for(m);
    PRG_HIP(h->size_source(cap));  // (all of the group or none of it, Mcap with it)
    PRG_TRY(ensure_motion(h));
    if (h->opt_sort_src)
        PRG_TRY(morton_permutation(h, source_hd, m, dim, &h->perm_src, &h->sext2));
    else
        h->perm_src.release();
    PRG_TRY(prg::ensure_stage(h, (size_t)m * dim * sizeof(float)));
    PRG_HIP(hipMemcpyAsync(h->stage.p, source_hd, (size_t)m * dim * sizeof(float), hipMemcpyDefault, h->stream));
    k_pack_cloud<<<grid1(cap), kBlock, 0, h->stream>>>((const float*)h->stage.p, m, dim, h->src4.p, cap, prg::kSrcPad,
                                                       0.f, h->perm_src.p);
    k_pack_cloud<<<grid1(cap), kBlock, 0, h->stream>>>((const float*)h->stage.p, m, dim, h->z4.p, cap, prg::kSrcPad, 0.f,
                                                       h->perm_src.p);
    // boxes of the whole padded array once; the per-iteration transform kernel refreshes the blocks with real points
    k_group_meta<<<grid1(cap / prg::kGroup), kBlock, 0, h->stream>>>(h->z4.p, cap / prg::kGroup, h->zmeta.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));  // the caller's buffer may be pageable host memory
    h->M = m;
    h->D = dim;
    h->have_colmin = false;
    h->have_source = true;
    return PRG_OK;
}

int prg_cpd_set_source_weights(prg_cpd* h, const double* log_weights_hd, double uniform_ratio) {
    PRG_REQUIRE(h && h->have_source, PRG_ERR_STATE, "prg_cpd_set_source_weights: source not set");
    PRG_REQUIRE(uniform_ratio >= 0.0, PRG_ERR_INVALID, "prg_cpd_set_source_weights: uniform_ratio must be >= 0");
    PRG_ENTER(h->device);
    h->uniform_ratio = uniform_ratio;
    h->estep_state_live = false;
    if (!log_weights_hd) {
        PRG_HIP(hipStreamSynchronize(h->stream));
        h->srcw.release();
        return PRG_OK;
    }
    hipPointerAttribute_t attr;
    const bool on_host = hipPointerGetAttributes(&attr, log_weights_hd) != hipSuccess || attr.type != hipMemoryTypeDevice;
    (void)hipGetLastError();
    if (on_host)  // a_m > 1 would make q_m negative and break the cull bounds: normalise by the largest weight first
        for (int64_t i = 0; i < h->M; ++i)
            PRG_REQUIRE(log_weights_hd[i] <= 0.0, PRG_ERR_INVALID,
                        "prg_cpd_set_source_weights: log-weight %lld is %g, must be <= 0 (and not NaN)", (long long)i,
                        log_weights_hd[i]);
    if (!h->srcw.p) PRG_HIP(h->srcw.reset(h->Mcap));
    PRG_TRY(prg::ensure_stage(h, (size_t)h->M * sizeof(double)));
    PRG_HIP(hipMemcpyAsync(h->stage.p, log_weights_hd, (size_t)h->M * sizeof(double), hipMemcpyDefault, h->stream));
    k_gather_weights<<<grid1(h->M), kBlock, 0, h->stream>>>((const double*)h->stage.p, h->M, h->perm_src.p, h->srcw.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_colmin = false;
    return PRG_OK;
}

int prg_cpd_set_target(prg_cpd* h, const float* target_hd, int64_t n_local, int dim, int64_t n_global) {
    PRG_REQUIRE(h && target_hd, PRG_ERR_INVALID, "prg_cpd_set_target: NULL argument");
    PRG_REQUIRE(n_local > 0 && n_global >= n_local && (dim == 2 || dim == 3), PRG_ERR_INVALID,
                "prg_cpd_set_target: need 0 < n_local <= n_global and dim in {2,3}");
    PRG_REQUIRE(!h->have_source || h->D == dim, PRG_ERR_INVALID,
                "prg_cpd_set_target: dim %d does not match source dim %d", dim, h->D);
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_target = h->have_estep = h->estep_state_live = false;  // (as in prg_cpd_set_source)
    // (the sums of the previous target no longer describe this one: no lean row pass until prg_cpd_init_sums has run)
    if (h->tsum_local) PRG_HIP(hipMemsetAsync(h->tsum_local, 0, 4 * sizeof(double), h->stream));
    const int64_t cap = cap_for(n_local);
    bool fresh = false;
    PRG_HIP(h->size_target(cap, &fresh));
    if (fresh) PRG_HIP(hipMemsetAsync(h->colmin.p, 0, (size_t)h->colmin.cap * sizeof(float), h->stream));
    PRG_TRY(ensure_motion(h));
    if (h->opt_sort_tgt)
        PRG_TRY(morton_permutation(h, target_hd, n_local, dim, &h->perm_tgt, &h->text2, h->tbox));
    else
        h->perm_tgt.release();
    PRG_TRY(prg::ensure_stage(h, (size_t)n_local * dim * sizeof(float)));
    PRG_HIP(hipMemcpyAsync(h->stage.p, target_hd, (size_t)n_local * dim * sizeof(float), hipMemcpyDefault, h->stream));
    k_pack_cloud<<<grid1(cap), kBlock, 0, h->stream>>>((const float*)h->stage.p, n_local, dim, h->tgt4.p, cap,
                                                       prg::kTgtPad, 0.f, h->perm_tgt.p);
    // the target never moves: its group boxes are written once (k_colfinal refreshes the b_n range)
    k_group_meta<<<grid1(cap / prg::kGroup), kBlock, 0, h->stream>>>(h->tgt4.p, cap / prg::kGroup, h->tmeta.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->N = n_local;
    h->Nglobal = n_global;
    h->D = dim;
    h->have_colmin = false;
    h->have_target = true;
    return PRG_OK;
}

int prg_cpd_bind_moments(prg_cpd* h, double* moments_dev) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_bind_moments: NULL handle");
    h->moments = moments_dev ? moments_dev : h->state.p;
    return PRG_OK;
}

int prg_cpd_moments_ptr(prg_cpd* h, double** moments_dev) {
    PRG_REQUIRE(h && moments_dev, PRG_ERR_INVALID, "prg_cpd_moments_ptr: NULL argument");
    *moments_dev = h->moments;
    return PRG_OK;
}

int prg_cpd_params_ptr(prg_cpd* h, double** params_dev) {
    PRG_REQUIRE(h && params_dev, PRG_ERR_INVALID, "prg_cpd_params_ptr: NULL argument");
    *params_dev = h->params;
    return PRG_OK;
}

int prg_cpd_set_tuning(prg_cpd* h, int r_col, int seg_col, int r_row, int seg_row) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_tuning: NULL handle");
    auto ok_r = [](int r) { return r == 0 || r == 2 || r == 4 || r == -2 || r == -4; };
    PRG_REQUIRE(ok_r(r_col) && ok_r(r_row), PRG_ERR_INVALID,
                "prg_cpd_set_tuning: points per lane must be 0 (auto), 2, 4 (packed) or -2, -4 (scalar form)");
    PRG_REQUIRE(seg_col >= 0 && seg_col <= 1024 && seg_row >= 0 && seg_row <= 256, PRG_ERR_INVALID,
                "prg_cpd_set_tuning: segment counts must be in [0, 1024] (column pass) / [0, 256] (row pass)");
    h->r_col = r_col;
    h->seg_col = seg_col;
    h->r_row = r_row;
    h->seg_row = seg_row;
    return PRG_OK;
}

int prg_cpd_set_dense_engine(prg_cpd* h, int mode, double bound) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_dense_engine: NULL handle");
    PRG_REQUIRE(mode >= 0 && mode <= 2, PRG_ERR_INVALID, "prg_cpd_set_dense_engine: mode must be 0, 1 or 2");
    PRG_REQUIRE(bound >= 0.0, PRG_ERR_INVALID, "prg_cpd_set_dense_engine: bound must be >= 0 (0 keeps the default)");
    h->dense_engine = mode;
    if (bound > 0.0) h->dense_bound = bound;
    // the switch starts over on the new engine mode; unlike a new registration (prg_cpd_init_params) this keeps what describes the
    // sweeps already run - the last E-step was the fused sweep, the matrix-core grid is cut fine - as it always has
    EngineSwitch fresh;
    fresh.pred_fused = h->eng.pred_fused;
    fresh.grid_fine = h->eng.grid_fine;
    h->eng = fresh;
    return PRG_OK;
}

int prg_cpd_last_estep_engine(prg_cpd* h, int* engine) {
    PRG_REQUIRE(h && engine, PRG_ERR_INVALID, "prg_cpd_last_estep_engine: NULL argument");
    *engine = h->last_estep_mfma ? 1 : 0;
    return PRG_OK;
}

int prg_cpd_set_sparse_engine(prg_cpd* h, int mode) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_sparse_engine: NULL handle");
    PRG_REQUIRE(mode >= 0 && mode <= 3, PRG_ERR_INVALID, "prg_cpd_set_sparse_engine: mode must be 0 (grid of culled waves), 1 (default: owner sweep for single-sweep "
                "iterations, work queue for the two-sweep E-steps of large clouds), 2 (work queue always) or 3 (round 5's default: queue for large clouds, no owner sweep)");
    h->sparse_engine = mode;
    return PRG_OK;
}

int prg_cpd_last_estep_engines(prg_cpd* h, int* col_engine, int* row_engine) {
    PRG_REQUIRE(h && col_engine && row_engine, PRG_ERR_INVALID, "prg_cpd_last_estep_engines: NULL argument");
    *col_engine = h->last_estep_mfma ? 1 : 0;
    *row_engine = h->last_estep_row_mfma ? 1 : 0;
    return PRG_OK;
}

int prg_cpd_last_estep_lean(prg_cpd* h, int* lean) {
    PRG_REQUIRE(h && lean, PRG_ERR_INVALID, "prg_cpd_last_estep_lean: NULL argument");
    *lean = h->last_estep_row_lean ? 1 : 0;
    return PRG_OK;
}

int prg_cpd_set_moments_only(prg_cpd* h, int mode) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_moments_only: NULL handle");
    PRG_REQUIRE(mode >= 0 && mode <= 2, PRG_ERR_INVALID, "prg_cpd_set_moments_only: mode must be 0, 1 or 2");
    h->moments_only = mode == 1;
    h->fused_in_iterate = mode != 2;
    return PRG_OK;
}

int prg_cpd_set_resid_sweep(prg_cpd* h, int on) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_resid_sweep: NULL handle");
    h->resid_sweep = on != 0;
    return PRG_OK;
}

int prg_cpd_set_fused_factor(prg_cpd* h, double factor) {
    PRG_REQUIRE(h && factor >= 0.0, PRG_ERR_INVALID, "prg_cpd_set_fused_factor: need a handle and a factor >= 0");
    h->fused_factor = factor;
    return PRG_OK;
}

int prg_cpd_last_estep_fused(prg_cpd* h, int* fused) {
    PRG_REQUIRE(h && fused, PRG_ERR_INVALID, "prg_cpd_last_estep_fused: NULL argument");
    *fused = h->last_estep_fused ? 1 : 0;
    return PRG_OK;
}

int prg_cpd_set_stream_mode(prg_cpd* h, int on) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_stream_mode: NULL handle");
    h->mfma_stream = on != 0;
    return PRG_OK;
}

int prg_cpd_set_lean_factor(prg_cpd* h, double factor) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_lean_factor: NULL handle");
    h->lean_factor = factor;
    return PRG_OK;
}

int prg_cpd_set_options(prg_cpd* h, int sort_source, int sort_target, int cull) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_options: NULL handle");
    PRG_REQUIRE(!h->have_source && !h->have_target, PRG_ERR_STATE,
                "prg_cpd_set_options: must be called before the clouds are uploaded");
    h->opt_sort_src = sort_source != 0;
    h->opt_sort_tgt = sort_target != 0;
    h->opt_cull = cull != 0;
    return PRG_OK;
}

int prg_cpd_init_sums(prg_cpd* h) {
    PRG_REQUIRE(h && h->have_target, PRG_ERR_STATE, "prg_cpd_init_sums: target not set");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_mompart(h));
    const int nblk = (int)prg::ceil_div(h->N, kBlock);
    k_zero_doubles<<<1, 64, 0, h->stream>>>(h->moments, PRG_NMOMENTS);
    k_cloud_sums<<<nblk, kBlock, 0, h->stream>>>(h->tgt4.p, h->N, h->mompart.p);
    prg::reduce_partials(h, h->mompart.p, nblk, 4, h->moments, 24);
    PRG_HIP(hipGetLastError());
    PRG_TRY(prg::ensure_engine_state(h));
    PRG_HIP(hipMemcpyAsync(h->tsum_local, h->moments + 24, 4 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (h->comm) PRG_TRY(prg::comm_all_reduce_f64(h->comm, h->moments, PRG_NMOMENTS, h->stream));  // (after the LOCAL sums were kept)
    return PRG_OK;
}

int prg_cpd_set_comm(prg_cpd* h, prg_comm* comm) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_set_comm: NULL handle");
    PRG_REQUIRE(!comm || comm->device == h->device, PRG_ERR_INVALID, "prg_cpd_set_comm: the communicator lives on device %d, the plan on %d",
                comm ? comm->device : -1, h->device);
    h->comm = comm;
    return PRG_OK;
}

// R^T R = I to 1e-12 for the row-major 3 x 3 block at `lin` (what the fused single sweep's frame change assumes)
static bool is_rotation(const double* lin) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += lin[3 * k + i] * lin[3 * k + j];
            if (!(fabs(d - (i == j ? 1.0 : 0.0)) <= 1.0e-12)) return false;
        }
    return true;
}

int prg_cpd_init_params(prg_cpd* h, const double* init_params_host) {
    PRG_REQUIRE(h && h->have_source && h->have_target, PRG_ERR_STATE, "prg_cpd_init_params: clouds not set");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_mompart(h));
    const int nblk = (int)prg::ceil_div(h->M, kBlock);
    double* srcsum = prg::mom_scratch(*h);
    double* init_dev = nullptr;
    if (init_params_host) {
        init_dev = srcsum + 8;
        PRG_HIP(hipMemcpyAsync(init_dev, init_params_host, 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    k_cloud_sums<<<nblk, kBlock, 0, h->stream>>>(h->src4.p, h->M, h->mompart.p);
    prg::reduce_partials(h, h->mompart.p, nblk, 4, srcsum, 0);
    k_init_params<<<1, 64, 0, h->stream>>>(h->moments, srcsum, h->params, (double)h->M, (double)h->Nglobal, h->D,
                                           init_dev);
    PRG_HIP(hipGetLastError());
    if (init_params_host) PRG_HIP(hipStreamSynchronize(h->stream));  // host buffer may be reused by the caller
    h->have_colmin = false;  // a new registration starts: its first column pass takes no seed from the previous one
    h->estep_state_live = false;
    h->eng = EngineSwitch();  // ... and it starts in the dense regime, with nothing remembered
    // the fused single sweep maps its column-side sums back through s R: R has to be a rotation (the M-step's own results are)
    h->init_rot_orthonormal = !init_params_host || is_rotation(init_params_host);
    return PRG_OK;
}


int prg_cpd_engine_bounds(int64_t m, int64_t n_local, double* col_bound, double* row_bound) {
    PRG_REQUIRE(m > 0 && n_local > 0 && col_bound && row_bound, PRG_ERR_INVALID, "prg_cpd_engine_bounds: need m, n_local > 0 and two outputs");
    *col_bound = prg::engine_col_bound(m, n_local);
    *row_bound = prg::engine_row_bound(m, n_local);
    return PRG_OK;
}

int prg_cpd_estep(prg_cpd* h, double w) { return prg::estep_impl(h, w, nullptr); }

int prg_cpd_estep_timed(prg_cpd* h, double w, float* ms_out) {
    PRG_REQUIRE(h && ms_out, PRG_ERR_INVALID, "prg_cpd_estep_timed: NULL argument");
    PRG_ENTER(h->device);
    hipEvent_t ev[6];
    for (int i = 0; i < 6; ++i) PRG_HIP(hipEventCreate(&ev[i]));
    int st = prg::estep_impl(h, w, ev);
    if (st == PRG_OK) {
        hipError_t e = hipEventSynchronize(ev[5]);
        if (e != hipSuccess) {
            prg::set_error("prg_cpd_estep_timed: hipEventSynchronize failed: %s", hipGetErrorString(e));
            st = PRG_ERR_HIP;
        }
    }
    if (st == PRG_OK) {
        for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]);
        (void)hipEventElapsedTime(&ms_out[5], ev[0], ev[5]);
    }
    for (int i = 0; i < 6; ++i) (void)hipEventDestroy(ev[i]);
    return st;
}

int prg_cpd_pair_counts(prg_cpd* h, double* col_pairs, double* row_pairs) {
    PRG_REQUIRE(h && h->have_estep && col_pairs && row_pairs, PRG_ERR_STATE, "prg_cpd_pair_counts: no E-step has been run");
    PRG_ENTER(h->device);
    *col_pairs = h->dense_pairs_col;
    *row_pairs = h->dense_pairs_row;
    for (int pass = 0; pass < 2; ++pass) {  // sweeps over the work queue: one count of (128 x 32) blocks per unit
        const SweepQueue& q = pass ? h->qrow : h->qcol;
        if ((pass ? h->wg_row : h->wg_col) != -1) continue;
        int nu[2] = {0, 0};  // fine units [0, nu[0]), coarse units [cap_soft, cap_soft + nu[1])
        PRG_HIP(hipMemcpyAsync(nu, q.ctrl.p + 8, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
        double sum = 0.0;
        for (int part = 0; part < 2; ++part) {
            if (nu[part] <= 0) continue;
            std::vector<unsigned> host((size_t)nu[part]);
            PRG_HIP(hipMemcpyAsync(host.data(), q.ucount.p + (part ? q.cap_soft : 0), (size_t)nu[part] * sizeof(unsigned),
                                   hipMemcpyDeviceToHost, h->stream));
            PRG_HIP(hipStreamSynchronize(h->stream));
            for (int i = 0; i < nu[part]; ++i) sum += host[(size_t)i];
        }
        *(pass ? row_pairs : col_pairs) = sum * 128.0 * prg::kGroup;
    }
    if (h->wg_col > 0 || h->wg_row > 0) {
        std::vector<unsigned> host((size_t)h->wg_cap() * 2);
        PRG_HIP(hipMemcpyAsync(host.data(), h->wgcount.p, host.size() * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
        if (h->wg_col > 0) {
            double s = 0.0;
            for (int64_t i = 0; i < h->wg_col; ++i) s += host[(size_t)i];
            *col_pairs = s * h->wg_col_pairs;
        }
        if (h->wg_row > 0) {
            double s = 0.0;
            for (int64_t i = 0; i < h->wg_row; ++i) s += host[(size_t)(h->wg_cap() + i)];
            *row_pairs = s * h->wg_row_pairs;
        }
    }
    // counted blocks include the pad points that fill the last block of either cloud (C1: 1.00448e10 counted for 1e10 real
    // pairs in a dense sweep): never report more than the pairs there are
    const double all_pairs = (double)h->M * (double)h->N;
    *col_pairs = std::min(*col_pairs, all_pairs);
    *row_pairs = std::min(*row_pairs, all_pairs);
    return PRG_OK;
}

int prg_cpd_mstep(prg_cpd* h, int kind, int update_scale) {
    PRG_REQUIRE(h && h->have_source, PRG_ERR_STATE, "prg_cpd_mstep: source not set");
    PRG_REQUIRE(kind == PRG_TF_RIGID || kind == PRG_TF_AFFINE, PRG_ERR_INVALID,
                "prg_cpd_mstep: kind must be PRG_TF_RIGID or PRG_TF_AFFINE (use prg_cpd_mstep_nonrigid)");
    // a single-sweep E-step (fused / residual form) leaves tr(Y^T P1 Y) in MOMENTS[16] and zeros in [17..21]: enough for the rigid fit,
    // not for the affine one (cpd.py:230-235 needs all of Y^T diag(p1) Y)
    PRG_REQUIRE(kind == PRG_TF_RIGID || !(h->have_estep && h->last_estep_fused), PRG_ERR_STATE,
                "prg_cpd_mstep: the last E-step ran as the single sweep of a rigid iteration (prg_cpd_set_moments_only(1)): its "
                "moments do not hold Y^T diag(p1) Y, which the affine M-step needs");
    PRG_ENTER(h->device);
    k_mstep<<<1, 64, 0, h->stream>>>(h->moments, h->params, kind, update_scale, h->D);
    h->estep_state_live = false;  // sigma2 in PARAMS is the next E-step's now
    PRG_HIP(hipGetLastError());
    // the single sweeps map their column-side sums back through s R: only a rigid fit leaves a rotation in the parameter block
    h->init_rot_orthonormal = kind == PRG_TF_RIGID;
    return PRG_OK;
}

int prg_cpd_iterate(prg_cpd* h, int kind, int update_scale, double w, int n_iter) {
    PRG_REQUIRE(h && h->have_source && h->have_target, PRG_ERR_STATE, "prg_cpd_iterate: clouds not set");
    PRG_REQUIRE(kind == PRG_TF_RIGID || kind == PRG_TF_AFFINE, PRG_ERR_INVALID,
                "prg_cpd_iterate: kind must be PRG_TF_RIGID or PRG_TF_AFFINE");
    PRG_REQUIRE(n_iter >= 0, PRG_ERR_INVALID, "prg_cpd_iterate: n_iter must be >= 0");
    PRG_ENTER(h->device);
    // a rigid iteration wants nothing of its E-step but the moments: the dense regime may run the fused single sweep
    const bool keep = h->moments_only;
    if (kind == PRG_TF_RIGID && h->fused_in_iterate) h->moments_only = true;
    if (kind != PRG_TF_RIGID) h->moments_only = false;  // (an affine M-step needs all of Y^T diag(p1) Y: two sweeps, whatever the caller left set)
    int st = PRG_OK;
    for (int it = 0; it < n_iter && st == PRG_OK; ++it) {
        st = prg::estep_impl(h, w, nullptr);  // (ends with the all-reduce when a communicator is attached)
        if (st == PRG_OK) {
            k_mstep<<<1, 64, 0, h->stream>>>(h->moments, h->params, kind, update_scale, h->D);
            h->init_rot_orthonormal = kind == PRG_TF_RIGID;  // (an affine fit leaves a general B: no single sweeps from it)
        }
    }
    h->moments_only = keep;
    if (n_iter > 0) h->estep_state_live = false;  // (every iteration ends with an M-step)
    PRG_TRY(st);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int prg_cpd_get_params(prg_cpd* h, double* params_host) {
    PRG_REQUIRE(h && params_host, PRG_ERR_INVALID, "prg_cpd_get_params: NULL argument");
    PRG_ENTER(h->device);
    // through pinned memory: a device->host copy into pageable memory pays ~100 us of staging, and the EM driver
    // reads the parameter block every iteration when it has a tolerance to test
    PRG_HIP(h->pinned.ensure(64));
    PRG_HIP(hipMemcpyAsync(h->pinned.p, h->params, PRG_NPARAMS * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int* host_info = reinterpret_cast<int*>(h->pinned.p + 48);
    *host_info = 0;
    if (h->nr_info) PRG_HIP(hipMemcpyAsync(host_info, h->nr_info, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    for (int i = 0; i < PRG_NPARAMS; ++i) params_host[i] = h->pinned.p[i];
    if (*host_info != 0) {  // a non-rigid M-step since the last read-back hit a non-positive pivot (it does not stall to say so)
        const int pivot = *host_info - 1;
        PRG_HIP(hipMemsetAsync(h->nr_info, 0, sizeof(int), h->stream));
        prg::set_error("prg_cpd_mstep_nonrigid: the reduced system is not positive definite at pivot %d (sigma2 or lmd <= 0?)", pivot);
        return PRG_ERR_STATE;
    }
    return PRG_OK;
}

int prg_cpd_set_params(prg_cpd* h, const double* params_host) {
    PRG_REQUIRE(h && params_host, PRG_ERR_INVALID, "prg_cpd_set_params: NULL argument");
    PRG_ENTER(h->device);
    h->estep_state_live = false;
    PRG_HIP(hipMemcpyAsync(h->params, params_host, PRG_NPARAMS * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->init_rot_orthonormal = is_rotation(params_host);  // (a caller-set linear part that is no rotation keeps the two sweeps)
    return PRG_OK;
}

int prg_cpd_get_moments(prg_cpd* h, double* moments_host) {
    PRG_REQUIRE(h && moments_host, PRG_ERR_INVALID, "prg_cpd_get_moments: NULL argument");
    PRG_ENTER(h->device);
    // (not copy_out: the moments may live in memory the caller bound, prg_cpd_bind_moments, which no DevBuf describes)
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(hipMemcpy(moments_host, h->moments, PRG_NMOMENTS * sizeof(double), hipMemcpyDeviceToHost));
    return PRG_OK;
}

int prg_cpd_get_estep(prg_cpd* h, double* pt1_hd, double* p1_hd, double* px_hd) {
    PRG_REQUIRE(h && h->have_estep, PRG_ERR_STATE, "prg_cpd_get_estep: no E-step has been run");
    PRG_REQUIRE(h->rowacc_valid || (!p1_hd && !px_hd), PRG_ERR_STATE,
                "prg_cpd_get_estep: the last E-step ran as the fused single sweep of a rigid iteration (prg_cpd_iterate / "
                "prg_cpd_set_moments_only): it leaves MOMENTS and pt1, no per-point p1 / px");
    PRG_ENTER(h->device);
    const size_t need = (size_t)(h->N > h->M * h->D ? h->N : h->M * h->D) * sizeof(double);
    PRG_TRY(prg::ensure_stage(h, need));
    if (pt1_hd) {
        k_float_to_double<<<grid1(h->N), kBlock, 0, h->stream>>>(h->pt1.p, (double*)h->stage.p, h->N, h->perm_tgt.p);
        PRG_HIP(hipMemcpyAsync(pt1_hd, h->stage.p, h->N * sizeof(double), hipMemcpyDefault, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
    }
    if (p1_hd) {
        k_scatter_double<<<grid1(h->M), kBlock, 0, h->stream>>>(h->rowacc.p, (double*)h->stage.p, h->M, h->perm_src.p);
        PRG_HIP(hipMemcpyAsync(p1_hd, h->stage.p, h->M * sizeof(double), hipMemcpyDefault, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
    }
    if (px_hd) {
        k_pack_px<<<grid1(h->M), kBlock, 0, h->stream>>>(h->rowacc.p, h->Mcap, h->M, h->D, (double*)h->stage.p, h->perm_src.p);
        PRG_HIP(hipMemcpyAsync(px_hd, h->stage.p, h->M * h->D * sizeof(double), hipMemcpyDefault, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
    }
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int prg_cpd_get_tsource(prg_cpd* h, float* tsource_hd) {
    PRG_REQUIRE(h && h->have_source && tsource_hd, PRG_ERR_STATE, "prg_cpd_get_tsource: source not set");
    PRG_ENTER(h->device);
    PRG_TRY(prg::ensure_stage(h, (size_t)h->M * h->D * sizeof(float)));
    k_unpack_points<<<grid1(h->M), kBlock, 0, h->stream>>>(h->z4.p, h->M, h->D, (float*)h->stage.p, h->perm_src.p);
    PRG_HIP(hipMemcpyAsync(tsource_hd, h->stage.p, h->M * h->D * sizeof(float), hipMemcpyDefault, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    return PRG_OK;
}

int prg_cpd_moments_from_estep(prg_cpd* h, const double* pt1_hd, const double* p1_hd, const double* px_hd) {
    PRG_REQUIRE(h && h->have_source && h->have_target, PRG_ERR_STATE, "prg_cpd_moments_from_estep: clouds not set");
    PRG_REQUIRE(pt1_hd && p1_hd && px_hd, PRG_ERR_INVALID, "prg_cpd_moments_from_estep: NULL array");
    PRG_ENTER(h->device);
    const size_t nb_pt1 = (size_t)h->N * sizeof(double), nb_p1 = (size_t)h->M * sizeof(double),
                 nb_px = (size_t)h->M * h->D * sizeof(double);
    PRG_TRY(prg::ensure_stage(h, nb_pt1 + nb_p1 + nb_px));
    PRG_TRY(ensure_mompart(h));
    double* d_pt1 = (double*)h->stage.p;
    double* d_p1 = d_pt1 + h->N;
    double* d_px = d_p1 + h->M;
    PRG_HIP(hipMemcpyAsync(d_pt1, pt1_hd, nb_pt1, hipMemcpyDefault, h->stream));
    PRG_HIP(hipMemcpyAsync(d_p1, p1_hd, nb_p1, hipMemcpyDefault, h->stream));
    PRG_HIP(hipMemcpyAsync(d_px, px_hd, nb_px, hipMemcpyDefault, h->stream));
    const int nblk = prg::mom_blocks(*h);
    k_moments_from_arrays<<<nblk, kBlock, 0, h->stream>>>(d_pt1, d_p1, d_px, h->D, h->M, h->N, h->src4.p, h->tgt4.p,
                                                          h->perm_src.p, h->perm_tgt.p, h->mompart.p);
    prg::reduce_partials(h, h->mompart.p, nblk, kMomComp, h->moments, 0);
    k_rowacc_from_arrays<<<nblk, kBlock, 0, h->stream>>>(d_pt1, d_p1, d_px, h->D, h->M, h->N, h->Mcap, h->perm_src.p,
                                                         h->perm_tgt.p, h->rowacc.p, h->pt1.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_estep = true;  // rowacc / MOMENTS now hold an E-step result (the caller's): all 24 moments and the per-point block
    h->last_estep_fused = false;
    h->rowacc_valid = true;
    h->estep_state_live = false;  // (tgt4.w is not this result's b_n)
    return PRG_OK;
}

}  // extern "C"
