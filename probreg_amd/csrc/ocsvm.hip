// One-class nu-SVM with the RBF kernel: the feature generator of support-vector registration (reference
// probreg/features.py:72-100, which calls scikit-learn's svm.OneClassSVM(nu, kernel = "rbf", gamma), that is libsvm).
// Everything in fp64.  The dual in libsvm's scaling:
//
//   minimise 1/2 a' Q a   subject to 0 <= a_i <= 1, sum a_i = nu n,   Q_ij = exp(-gamma |x_i - x_j|^2)
//
// with the gradient G = Q a, the "up" set {a_i < 1}, the "low" set {a_i > 0}, m = max_up -G_i, M = min_low -G_i and
// libsvm's stop test m - M < tol.
//
// Working-set decomposition; every step is an ordinary launch on the handle's stream:
//   select      the points are dealt into kQ / 2 groups (index mod kQ / 2); every group hands in its most violating "up"
//               point and, the former excluded, its most violating "low" point.  The working set therefore holds the
//               globally maximal violating pair, so the gap of the working set is the gap of the whole problem, and its
//               kQ entries are distinct.  (Not the kQ most violating points overall: that needs a sort or a multi-pass
//               selection per round; the groups need one pass and no ordering of ties beyond "lowest index".)
//   subproblem  one workgroup, one thread per working-set variable, a and G of the set in registers, the points in LDS.
//               Second-order SMO with libsvm's WSS2 pair choice and clipping; kernel values are recomputed from the
//               points (two exp per thread and step), there is no kernel cache.  Stops at a local gap below
//               max(tol / 2, gap at entry / 10) or after inner_cap steps (host argument).
//   sweep       G_j += sum_w da_w k(x_w, x_j) over the working set, one thread per j, the set staged in LDS and walked in
//               slot order.  This is the kQ x n pair sweep, the part that grows with the cloud; the rows are consumed as
//               they are computed and never stored.
// The host reads one record per round (gap, steps, status) and ends the loop; no kernel waits on another workgroup and no
// device loop runs without a cap from the host.
//
// Determinism: no floating-point atomics, all reductions in a fixed order with ties going to the lowest index, so two
// solves of the same input give byte-identical a.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <new>
#include <vector>

#include "cell_grid.h"
#include "dev_buf.h"
#include "prg_common.h"

namespace {

constexpr int kQ = 256;           // working-set size = threads of the subproblem's workgroup (one wave per SIMD of a CU)
constexpr int kGroups = kQ / 2;   // groups of the selection: one "up" and one "low" pick each
constexpr int kBlock = 256;       // point-parallel kernels
constexpr double kTau = 1.0e-12;  // libsvm's TAU: floor of the pair's curvature

struct Rec {
    double gap;        // m - M of the whole problem when the round began (-inf: "up" or "low" is empty)
    double gap_after;  // gap of the working set when the subproblem stopped
    int inner;         // SMO steps taken
    int status;        // 1: gap < tol at entry, nothing was changed
};

__device__ inline double dist2(const double4 p, const double4 c) {
    const double dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
    return dx * dx + dy * dy + dz * dz;
}

// (ov, oi) beats (v, i): larger value, ties to the lower index; index < 0 means "none"
__device__ inline bool beats(double ov, int oi, double v, int i) {
    return oi >= 0 && (i < 0 || ov > v || (ov == v && oi < i));
}

// Best (value, index) of the workgroup (kQ = kBlock threads) in every thread.  sv / si: kQ / 64 entries of LDS.
__device__ inline void block_best(double& v, int& i, double* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (beats(ov, oi, v, i)) { v = ov; i = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    v = sv[0];
    i = si[0];
#pragma unroll
    for (int w = 1; w < kQ / 64; ++w)
        if (beats(sv[w], si[w], v, i)) { v = sv[w]; i = si[w]; }
}

// Group g = blockIdx.x holds the points g, g + kGroups, ...: ws[g] = its "up" point with the largest -G, ws[kGroups + g] =
// its "low" point with the smallest -G other than ws[g]; -1 where there is none.
__global__ __launch_bounds__(kBlock) void k_select(const double* __restrict__ alpha, const double* __restrict__ grad,
                                                   int64_t n, int* __restrict__ ws) {
    __shared__ double sv[kQ / 64];
    __shared__ int si[kQ / 64];
    const int g = blockIdx.x;
    double uv = 0.0;
    int ui = -1;
    for (int64_t i = g + (int64_t)threadIdx.x * kGroups; i < n; i += (int64_t)kBlock * kGroups)
        if (alpha[i] < 1.0 && beats(-grad[i], (int)i, uv, ui)) { uv = -grad[i]; ui = (int)i; }
    block_best(uv, ui, sv, si);
    double lv = 0.0;
    int li = -1;
    for (int64_t i = g + (int64_t)threadIdx.x * kGroups; i < n; i += (int64_t)kBlock * kGroups)
        if (alpha[i] > 0.0 && (int)i != ui && beats(grad[i], (int)i, lv, li)) { lv = grad[i]; li = (int)i; }
    block_best(lv, li, sv, si);
    if (threadIdx.x == 0) {
        ws[g] = ui;
        ws[kGroups + g] = li;
    }
}

// Second-order SMO on the working set (libsvm Solver::select_working_set / Solver::Solve with every y = +1, C = 1).
// Writes the new a of the set, d_idx / d_val = (point, change of a) per slot for the sweep, and the round's record.
__global__ __launch_bounds__(kQ) void k_subproblem(const double4* __restrict__ xs, double* __restrict__ alpha,
                                                   const double* __restrict__ grad, const int* __restrict__ ws,
                                                   double gamma, double tol, int inner_cap, int* __restrict__ d_idx,
                                                   double* __restrict__ d_val, Rec* __restrict__ rec) {
    __shared__ double4 sp[kQ];
    __shared__ double sv[kQ / 64];
    __shared__ int si[kQ / 64];
    __shared__ double pub[5];  // a_i, G_i, a_j, G_j, k_ij
    const int t = threadIdx.x;
    const int idx = ws[t];
    const bool valid = idx >= 0;
    const double4 p = valid ? xs[idx] : make_double4(0.0, 0.0, 0.0, 0.0);
    double a = valid ? alpha[idx] : 0.0, g = valid ? grad[idx] : 0.0;
    const double a0 = a;
    sp[t] = p;
    double gap0 = 0.0, gap = 0.0, eps = 0.0;
    int it = 0, status = 0;
    for (;;) {  // at most inner_cap steps
        double mv = -g;
        int mi = (valid && a < 1.0) ? t : -1;
        block_best(mv, mi, sv, si);  // m = max over "up" of -G
        double lv = g;
        int li = (valid && a > 0.0) ? t : -1;
        block_best(lv, li, sv, si);  // -M = max over "low" of G
        gap = (mi >= 0 && li >= 0) ? mv + lv : -INFINITY;
        if (it == 0) {
            gap0 = gap;
            status = !(gap >= tol);
            eps = fmax(0.5 * tol, 0.1 * gap0);
        }
        if (status || !(gap >= eps) || it >= inner_cap) break;
        // i = mi; j maximises b^2 / a_ij over the "low" points with b = m + G_j > 0 (WSS2)
        const double kit = exp(-gamma * dist2(p, sp[mi]));
        const double b = mv + g;
        double sc = 0.0;
        int sj = -1;
        if (valid && a > 0.0 && b > 0.0) {
            const double quad = 2.0 - 2.0 * kit;
            sc = b * b / (quad > 0.0 ? quad : kTau);
            sj = t;
        }
        block_best(sc, sj, sv, si);
        if (sj < 0) break;  // cannot happen while gap > 0: the "low" point that attains M has b = gap
        const double kjt = exp(-gamma * dist2(p, sp[sj]));
        if (t == mi) { pub[0] = a; pub[1] = g; }
        if (t == sj) { pub[2] = a; pub[3] = g; pub[4] = kit; }
        __syncthreads();
        const double ai = pub[0], gi = pub[1], aj = pub[2], gj = pub[3];
        double quad = 2.0 - 2.0 * pub[4];
        if (!(quad > 0.0)) quad = kTau;
        const double delta = (gi - gj) / quad;
        const double sum = ai + aj;
        double ni = ai - delta, nj = aj + delta;
        if (sum > 1.0) {
            if (ni > 1.0) { ni = 1.0; nj = sum - 1.0; }
        } else {
            if (nj < 0.0) { nj = 0.0; ni = sum; }
        }
        if (sum > 1.0) {
            if (nj > 1.0) { nj = 1.0; ni = sum - 1.0; }
        } else {
            if (ni < 0.0) { ni = 0.0; nj = sum; }
        }
        g = fma(ni - ai, kit, fma(nj - aj, kjt, g));
        if (t == mi) a = ni;
        if (t == sj) a = nj;
        ++it;  // (pub is next written after the two barriers of the next block_best)
    }
    d_idx[t] = idx;
    d_val[t] = valid ? a - a0 : 0.0;
    if (valid) alpha[idx] = a;
    if (t == 0) {
        rec->gap = gap0;
        rec->gap_after = gap;
        rec->inner = it;
        rec->status = status;
    }
}

// out_j (+)= sum_s coef_s exp(-gamma |t_j - x_{idx_s}|^2) over cnt sources in list order (idx == NULL: the first cnt points;
// idx_s < 0 or coef_s == 0: skipped).  rec != NULL: nothing to do when the round found the problem converged.
template <bool ACCUMULATE>
__global__ __launch_bounds__(kBlock) void k_sweep(const double4* __restrict__ tg, int64_t nt,
                                                  const double4* __restrict__ xs, const int* __restrict__ idx,
                                                  const double* __restrict__ coef, int64_t cnt, double gamma,
                                                  double* __restrict__ out, const Rec* __restrict__ rec) {
    __shared__ double4 sp[kBlock];
    __shared__ double sc[kBlock];
    if (rec != nullptr && rec->status != 0) return;
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = j < nt;
    const double4 p = live ? tg[j] : make_double4(0.0, 0.0, 0.0, 0.0);
    double acc = 0.0;
    for (int64_t s0 = 0; s0 < cnt; s0 += kBlock) {
        const int c = (int)min((int64_t)kBlock, cnt - s0);
        __syncthreads();
        if ((int)threadIdx.x < c) {
            const int64_t s = s0 + threadIdx.x;
            const int64_t id = idx ? (int64_t)idx[s] : s;
            sp[threadIdx.x] = id >= 0 ? xs[id] : make_double4(0.0, 0.0, 0.0, 0.0);
            sc[threadIdx.x] = id >= 0 ? coef[s] : 0.0;
        }
        __syncthreads();
        for (int q = 0; q < c; ++q) {
            const double w = sc[q];
            if (w != 0.0) acc = fma(w, exp(-gamma * dist2(p, sp[q])), acc);
        }
    }
    if (live) out[j] = ACCUMULATE ? out[j] + acc : acc;
}

}  // namespace

struct prg_ocsvm {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    int dim = 0;
    bool solved = false, profile = false;
    double gamma = 0.0, rho = 0.0, objective = 0.0;
    prg::DevBuf<double4> xs;          // the points group: xs, alpha, grad are [n], all there or none (n, dim say which)
    prg::DevBuf<double> alpha, grad;
    prg::DevBuf<int> sv_idx;          // the support list of the last solve and its coefficients
    prg::DevBuf<double> sv_coef;
    prg::DevBuf<int> ws, d_idx;       // [kQ] each, allocated once
    prg::DevBuf<double> d_val;
    prg::DevBuf<Rec> rec;
    std::vector<double> alpha_host;
    std::vector<int> support;
    double prof_ms[4] = {0.0, 0.0, 0.0, 0.0};  // initial gradient, select, subproblem, sweep
    struct Events {  // created by prg_ocsvm_set_profile, destroyed with the handle
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
        hipEvent_t& operator[](int i) { return e[i]; }
    } ev;
};

extern "C" {

int prg_ocsvm_create(prg_ocsvm** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_ocsvm_destroy(prg_ocsvm* h) {
    return prg::destroy_handle(h);
}

int prg_ocsvm_working_set_size(int* q_host) {
    PRG_REQUIRE(q_host != nullptr, PRG_ERR_INVALID, "prg_ocsvm_working_set_size: NULL argument");
    *q_host = kQ;
    return PRG_OK;
}

int prg_ocsvm_set_data(prg_ocsvm* h, const double* data_hd, int64_t n, int dim) {
    PRG_REQUIRE(h && data_hd, PRG_ERR_INVALID, "prg_ocsvm_set_data: NULL argument");
    PRG_REQUIRE(dim == 2 || dim == 3, PRG_ERR_INVALID, "prg_ocsvm_set_data: dim must be 2 or 3, got %d", dim);
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_ocsvm_set_data: need 1 <= n < 2^31 points");
    PRG_ENTER(h->device);
    std::vector<double> raw, pad;
    PRG_TRY(prg::load_cloud3(data_hd, n, dim, "prg_ocsvm_set_data: data contains NaN or infinity", raw, pad, nullptr, nullptr));
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->solved = false;
    h->n = 0;
    h->dim = 0;
    prg::release_all(h->sv_coef, h->sv_idx);
    hipError_t e = prg::reset_group(h->xs, n, h->alpha, n, h->grad, n);
    if (e == hipSuccess) e = h->ws.ensure(kQ, kQ);
    if (e == hipSuccess) e = h->d_idx.ensure(kQ, kQ);
    if (e == hipSuccess) e = h->d_val.ensure(kQ, kQ);
    if (e == hipSuccess) e = h->rec.ensure(1, 1);
    if (e == hipSuccess) e = hipMemcpyAsync(h->xs.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) prg::release_all(h->xs, h->alpha, h->grad);  // no half-built cloud: the handle is back to "no data"
    PRG_HIP(e);
    h->n = n;
    h->dim = dim;
    return PRG_OK;
}

int prg_ocsvm_set_profile(prg_ocsvm* h, int on) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ocsvm_set_profile: NULL argument");
    PRG_ENTER(h->device);
    if (on)
        for (hipEvent_t& e : h->ev.e)
            if (!e) PRG_HIP(hipEventCreate(&e));
    h->profile = on != 0;
    return PRG_OK;
}

int prg_ocsvm_get_profile(prg_ocsvm* h, double* ms4_host) {
    PRG_REQUIRE(h && ms4_host, PRG_ERR_INVALID, "prg_ocsvm_get_profile: NULL argument");
    for (int i = 0; i < 4; ++i) ms4_host[i] = h->prof_ms[i];
    return PRG_OK;
}

int prg_ocsvm_solve(prg_ocsvm* h, double gamma, double nu, double tol, int max_iter, int inner_cap, int* n_iter_host,
                    int* n_inner_host, int* converged_host, double* gap_host) {
    PRG_REQUIRE(h && n_iter_host && converged_host && gap_host, PRG_ERR_INVALID, "prg_ocsvm_solve: NULL argument");
    PRG_REQUIRE(h->xs.p != nullptr, PRG_ERR_STATE, "prg_ocsvm_solve: no data (prg_ocsvm_set_data first)");
    PRG_REQUIRE(gamma > 0.0 && std::isfinite(gamma), PRG_ERR_INVALID, "prg_ocsvm_solve: gamma must be > 0 and finite");
    PRG_REQUIRE(nu > 0.0 && nu <= 1.0, PRG_ERR_INVALID, "prg_ocsvm_solve: nu must lie in (0, 1]");
    PRG_REQUIRE(tol > 0.0 && std::isfinite(tol), PRG_ERR_INVALID, "prg_ocsvm_solve: tol must be > 0 and finite");
    PRG_REQUIRE(max_iter >= 0, PRG_ERR_INVALID, "prg_ocsvm_solve: max_iter must be >= 0");
    PRG_REQUIRE(inner_cap >= 1, PRG_ERR_INVALID, "prg_ocsvm_solve: inner_cap must be >= 1");
    PRG_ENTER(h->device);
    const int64_t n = h->n;
    const unsigned nb = (unsigned)prg::ceil_div(n, kBlock);
    h->solved = false;
    h->gamma = gamma;
    for (double& v : h->prof_ms) v = 0.0;
    // libsvm's start (svm.cpp solve_one_class): the first floor(nu n) points at the bound, the next takes the rest
    h->alpha_host.assign((size_t)n, 0.0);
    const int64_t n_full = std::min<int64_t>((int64_t)(nu * (double)n), n);
    for (int64_t i = 0; i < n_full; ++i) h->alpha_host[(size_t)i] = 1.0;
    if (n_full < n) h->alpha_host[(size_t)n_full] = nu * (double)n - (double)n_full;
    const int64_t n_start = std::min<int64_t>(n_full + 1, n);
    PRG_HIP(hipMemcpyAsync(h->alpha.p, h->alpha_host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (h->profile) PRG_HIP(hipEventRecord(h->ev[0], h->stream));
    k_sweep<false><<<nb, kBlock, 0, h->stream>>>(h->xs.p, n, h->xs.p, nullptr, h->alpha.p, n_start, gamma, h->grad.p, nullptr);
    PRG_HIP(hipGetLastError());
    if (h->profile) {
        PRG_HIP(hipEventRecord(h->ev[1], h->stream));
        PRG_HIP(hipEventSynchronize(h->ev[1]));
        float ms = 0.0f;
        PRG_HIP(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->prof_ms[0] = ms;
    }
    int rounds = 0, conv = 0;
    int64_t inner = 0;
    Rec rec{};
    for (;;) {  // at most max_iter rounds, then one evaluation of the gap that changes nothing
        const bool step = rounds < max_iter;
        if (h->profile) PRG_HIP(hipEventRecord(h->ev[0], h->stream));
        k_select<<<kGroups, kBlock, 0, h->stream>>>(h->alpha.p, h->grad.p, n, h->ws.p);
        PRG_HIP(hipGetLastError());
        if (h->profile) PRG_HIP(hipEventRecord(h->ev[1], h->stream));
        k_subproblem<<<1, kQ, 0, h->stream>>>(h->xs.p, h->alpha.p, h->grad.p, h->ws.p, gamma, tol, step ? inner_cap : 0, h->d_idx.p,
                                              h->d_val.p, h->rec.p);
        PRG_HIP(hipGetLastError());
        if (h->profile) PRG_HIP(hipEventRecord(h->ev[2], h->stream));
        if (step) {
            k_sweep<true><<<nb, kBlock, 0, h->stream>>>(h->xs.p, n, h->xs.p, h->d_idx.p, h->d_val.p, kQ, gamma, h->grad.p, h->rec.p);
            PRG_HIP(hipGetLastError());
        }
        if (h->profile) PRG_HIP(hipEventRecord(h->ev[3], h->stream));
        PRG_HIP(hipMemcpyAsync(&rec, h->rec.p, sizeof(Rec), hipMemcpyDeviceToHost, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
        if (h->profile)
            for (int i = 0; i < 3; ++i) {
                float ms = 0.0f;
                PRG_HIP(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
                h->prof_ms[i + 1] += ms;
            }
        if (rec.status) {
            conv = 1;
            break;
        }
        if (!step) break;
        ++rounds;
        inner += rec.inner;
    }
    // rho (libsvm Solver::calculate_rho with y = +1), the objective and the support list, on the host in index order
    std::vector<double> grad((size_t)n);
    PRG_HIP(hipMemcpyAsync(h->alpha_host.data(), h->alpha.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipMemcpyAsync(grad.data(), h->grad.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    double ub = std::numeric_limits<double>::infinity(), lb = -ub, sum_free = 0.0, obj = 0.0;
    int64_t n_free = 0;
    h->support.clear();
    std::vector<double> coef;
    for (int64_t i = 0; i < n; ++i) {
        const double a = h->alpha_host[(size_t)i], gi = grad[(size_t)i];
        if (a >= 1.0) {
            lb = std::max(lb, gi);
        } else if (a <= 0.0) {
            ub = std::min(ub, gi);
        } else {
            ++n_free;
            sum_free += gi;
        }
        if (a > 0.0) {
            h->support.push_back((int)i);
            coef.push_back(a);
            obj += a * gi;
        }
    }
    h->rho = n_free > 0 ? sum_free / (double)n_free : 0.5 * (ub + lb);
    h->objective = 0.5 * obj;
    PRG_HIP(prg::reset_group(h->sv_idx, (int64_t)h->support.size(), h->sv_coef, (int64_t)coef.size()));
    PRG_HIP(hipMemcpyAsync(h->sv_idx.p, h->support.data(), h->support.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    PRG_HIP(hipMemcpyAsync(h->sv_coef.p, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->solved = true;
    *n_iter_host = rounds;
    if (n_inner_host) *n_inner_host = (int)std::min<int64_t>(inner, std::numeric_limits<int>::max());
    *converged_host = conv;
    *gap_host = rec.gap;
    return PRG_OK;
}

int prg_ocsvm_get_solution(prg_ocsvm* h, double* alpha_host, double* rho_host, double* objective_host, int* n_support_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_ocsvm_get_solution: NULL argument");
    PRG_REQUIRE(h->solved, PRG_ERR_STATE, "prg_ocsvm_get_solution: prg_ocsvm_solve first");
    if (alpha_host) std::copy(h->alpha_host.begin(), h->alpha_host.end(), alpha_host);
    if (rho_host) *rho_host = h->rho;
    if (objective_host) *objective_host = h->objective;
    if (n_support_host) *n_support_host = (int)h->support.size();
    return PRG_OK;
}

int prg_ocsvm_get_support(prg_ocsvm* h, int* index_host) {
    PRG_REQUIRE(h && index_host, PRG_ERR_INVALID, "prg_ocsvm_get_support: NULL argument");
    PRG_REQUIRE(h->solved, PRG_ERR_STATE, "prg_ocsvm_get_support: prg_ocsvm_solve first");
    std::copy(h->support.begin(), h->support.end(), index_host);
    return PRG_OK;
}

int prg_ocsvm_decision(prg_ocsvm* h, const double* points_hd, int64_t k, double* out_hd) {
    PRG_REQUIRE(h && points_hd && out_hd, PRG_ERR_INVALID, "prg_ocsvm_decision: NULL argument");
    PRG_REQUIRE(h->solved, PRG_ERR_STATE, "prg_ocsvm_decision: prg_ocsvm_solve first");
    PRG_REQUIRE(k >= 1 && k < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_ocsvm_decision: need 1 <= k < 2^31 points");
    PRG_ENTER(h->device);
    std::vector<double> raw, pad;
    PRG_TRY(prg::load_cloud3(points_hd, k, h->dim, "prg_ocsvm_decision: points contain NaN or infinity", raw, pad, nullptr, nullptr));
    prg::DevBuf<double4> tg;
    prg::DevBuf<double> out;
    PRG_HIP(tg.reset(k));
    if (out.reset(k) != hipSuccess) {
        prg::set_error("prg_ocsvm_decision: out of device memory");
        return PRG_ERR_HIP;
    }
    PRG_HIP(hipMemcpyAsync(tg.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_sweep<false><<<(unsigned)prg::ceil_div(k, kBlock), kBlock, 0, h->stream>>>(
        tg.p, k, h->xs.p, h->sv_idx.p, h->sv_coef.p, (int64_t)h->support.size(), h->gamma, out.p, nullptr);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    PRG_HIP(hipMemcpy(out_hd, out.p, (size_t)k * sizeof(double), hipMemcpyDefault));
    return PRG_OK;
}

}  // extern "C"
