// Spherical Gaussian-mixture fit of a point cloud: the feature generator of GMMReg (reference probreg/features.py:54-69,
// which calls scikit-learn's GaussianMixture(n_components = K, covariance_type = "spherical")).  Everything in fp64.
//
// Three stages, each an entry point of its own:
//   seed   greedy k-means++ (Arthur & Vassilvitskii 2007; 2 + floor(log K) candidates per step, the one that lowers the
//          potential most is kept).  The uniforms come from the host, all sampling runs on the device.
//   lloyd  Lloyd iterations from the seeds until no label changes or the summed squared centre shift <= tol.
//   em     EM from the current parameters (set explicitly or derived from the Lloyd labels), restating scikit-learn:
//          log p(i, k) = log w_k + dim log c_k - dim/2 log 2 pi - c_k^2 |x_i - mu_k|^2 / 2  with  c_k = 1 / sqrt(cov_k),
//          the per-point normaliser by log-sum-exp, nk = sum resp + 10 eps, means = sum resp x / nk,
//          cov = mean_d(sum resp x_d^2 / nk - means_d^2 + reg_covar), weights = nk / sum nk, lower bound = mean normaliser.
//
// Sweeps.  The N x K responsibilities are never stored.  The normaliser sweep has one thread per point that walks the
// components twice (maximum, then sum of exponentials); the component records are wave-uniform reads.  The moment sweep
// has one thread per component that walks a chunk of points staged in LDS and recomputes exp(log p - normaliser).
//
// Determinism: no floating-point atomics.  A component's sums over a chunk of points are accumulated by one thread in
// point order, the chunks are added in chunk order, sums over components and over workgroups run in a fixed tree, so a
// fit is byte-repeatable.  The differences x - mu are formed directly (scikit-learn expands the square).
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

constexpr int kBlock = 256;      // point-parallel kernels
constexpr int kCompBlock = 128;  // components per workgroup of the moment sweep (= points per LDS tile)
constexpr int kSeedChunk = 256;  // points per potential partial of the seeding (= kBlock)
constexpr int kMaxTrials = 16;   // candidates per k-means++ step (one wave each in k_seed_choose)
constexpr int kChooseThreads = 1024;
constexpr int kRec = 8;          // doubles per component record: mu (3), -c^2 / 2, log w + dim log c - dim/2 log 2 pi
constexpr int kMom = 8;          // doubles per component moment: sum r, sum r x (3), sum r x^2 (3), unused
constexpr int kMaxMomChunks = 512;
constexpr double kLog2Pi = 1.8378770664093453;
constexpr double kTenEps = 10.0 * 2.220446049250313e-16;  // 10 * np.finfo(float64).eps

enum { kFinNormalise = 0, kFinInit = 1 };

__device__ inline double dist2(const double4 p, const double4 c) {
    const double dx = p.x - c.x, dy = p.y - c.y, dz = p.z - c.z;
    return dx * dx + dy * dy + dz * dz;
}

// Fixed-order sum over the workgroup (tree in LDS); the result is in red[0] after the call.
template <int NT>
__device__ inline void block_tree_sum(double* red) {
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
}

// ---- seeding ----------------------------------------------------------------------------------------------------------
// Applies centre `prev` to the running minimum squared distance, then the potential of every candidate over this
// workgroup's chunk: part[chunk][l] = sum_i min(mind2_i, |x_i - x_cand[l]|^2); without candidates part[chunk][0] = sum mind2.
__global__ __launch_bounds__(kBlock) void k_seed_sweep(const double4* __restrict__ xs, int64_t n,
                                                       const int* __restrict__ centers, int prev,
                                                       const int* __restrict__ cand, int ncand,
                                                       double* __restrict__ mind2, double* __restrict__ part) {
    __shared__ double red[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    double4 p = make_double4(0.0, 0.0, 0.0, 0.0);
    double m = 0.0;
    if (live) {
        p = xs[i];
        m = fmin(mind2[i], dist2(p, xs[centers[prev]]));
        mind2[i] = m;
    }
    const int nv = ncand > 0 ? ncand : 1;
    for (int l = 0; l < nv; ++l) {
        double v = m;
        if (ncand > 0 && live) v = fmin(m, dist2(p, xs[cand[l]]));
        __syncthreads();
        red[threadIdx.x] = live ? v : 0.0;
        block_tree_sum<kBlock>(red);
        if (threadIdx.x == 0) part[(int64_t)blockIdx.x * kMaxTrials + l] = red[0];
    }
}

// One workgroup: the candidate with the lowest potential becomes centre s (first minimum), then the candidates of step
// s + 1 are drawn with probability proportional to the updated squared distances: an inclusive prefix over the chunk
// partials of the winner (which are the chunk sums of the updated distances), a search for the chunk and one wave per
// candidate that scans the 256 points of its chunk.
__global__ __launch_bounds__(kChooseThreads) void k_seed_choose(const double4* __restrict__ xs, int64_t n,
                                                                const double* __restrict__ mind2,
                                                                const double* __restrict__ part, int nc, int ncand,
                                                                int* __restrict__ cand, int* __restrict__ centers, int s,
                                                                int k, const double* __restrict__ unif, int trials,
                                                                double* __restrict__ pre) {
    __shared__ double red[kChooseThreads];
    __shared__ double tot[kMaxTrials];
    __shared__ int best_s;
    const int t = threadIdx.x;
    if (ncand > 0) {
        for (int l = 0; l < ncand; ++l) {
            double a = 0.0;
            for (int c = t; c < nc; c += kChooseThreads) a += part[(int64_t)c * kMaxTrials + l];
            __syncthreads();
            red[t] = a;
            block_tree_sum<kChooseThreads>(red);
            if (t == 0) tot[l] = red[0];
        }
        if (t == 0) {
            int b = 0;
            for (int l = 1; l < ncand; ++l)
                if (tot[l] < tot[b]) b = l;
            best_s = b;
            centers[s] = cand[b];
        }
    } else if (t == 0) {
        best_s = 0;
    }
    __syncthreads();
    if (s + 1 >= k) return;
    const int best = best_s;
    const int center = centers[s];
    // inclusive prefix of the winner's chunk sums: per-thread runs, a Hillis-Steele scan of the run totals, runs again
    const int per = (nc + kChooseThreads - 1) / kChooseThreads;
    const int c0 = min(t * per, nc), c1 = min(c0 + per, nc);
    double local = 0.0;
    for (int c = c0; c < c1; ++c) local += part[(int64_t)c * kMaxTrials + best];
    __syncthreads();
    red[t] = local;
    __syncthreads();
    for (int o = 1; o < kChooseThreads; o <<= 1) {
        const double v = (t >= o) ? red[t - o] : 0.0;
        __syncthreads();
        red[t] += v;
        __syncthreads();
    }
    double run = red[t] - local;
    for (int c = c0; c < c1; ++c) {
        run += part[(int64_t)c * kMaxTrials + best];
        pre[c] = run;
    }
    __syncthreads();
    const double total = red[kChooseThreads - 1];
    const int wave = t >> 6, lane = t & 63;
    if (wave >= trials) return;
    const double target = unif[(int64_t)(s + 1) * trials + wave] * total;
    int lo = 0, hi = nc - 1;  // first chunk whose inclusive prefix reaches the target (the last one if none does)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid] >= target) hi = mid; else lo = mid + 1;
    }
    const int c = lo;
    const double rest = target - (c > 0 ? pre[c - 1] : 0.0);
    const double4 cp = xs[center];
    double v[4], sum = 0.0;
    const int64_t i0 = (int64_t)c * kSeedChunk + lane * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j;
        v[j] = (i < n) ? fmin(mind2[i], dist2(xs[i], cp)) : 0.0;
        sum += v[j];
    }
    double incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    const unsigned long long hit = __ballot(incl >= rest);
    int64_t pick = min((int64_t)c * kSeedChunk + kSeedChunk - 1, n - 1);
    if (hit != 0ull) {
        const int first = __ffsll((long long)hit) - 1;
        if (lane == first) {
            double acc = incl - sum;
            int j = 0;
            for (; j < 3; ++j) {
                acc += v[j];
                if (acc >= rest) break;
            }
            cand[wave] = (int)min(i0 + j, n - 1);
        }
    } else if (lane == 0) {
        cand[wave] = (int)pick;
    }
}

__global__ __launch_bounds__(kBlock) void k_fill(double* __restrict__ a, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) a[i] = v;
}

__global__ __launch_bounds__(kBlock) void k_gather_centers(const double4* __restrict__ xs, const int* __restrict__ centers,
                                                           int k, double* __restrict__ mu) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= k) return;
    const double4 p = xs[centers[j]];
    mu[3 * j] = p.x;
    mu[3 * j + 1] = p.y;
    mu[3 * j + 2] = p.z;
}

// ---- Lloyd ------------------------------------------------------------------------------------------------------------
// label = nearest centre (first minimum); counts the labels that changed (an integer atomic: exact in any order).
__global__ __launch_bounds__(kBlock) void k_assign(const double4* __restrict__ xs, int64_t n, const double* __restrict__ mu,
                                                   int k, int* __restrict__ labels, int* __restrict__ n_changed) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double4 p = xs[i];
    double bd = INFINITY;
    int best = 0;
    for (int j = 0; j < k; ++j) {
        const double dx = p.x - mu[3 * j], dy = p.y - mu[3 * j + 1], dz = p.z - mu[3 * j + 2];
        const double d = dx * dx + dy * dy + dz * dz;
        if (d < bd) { bd = d; best = j; }
    }
    if (labels[i] != best) {
        labels[i] = best;
        atomicAdd(n_changed, 1);
    }
}

// New centres from the label moments (an empty cluster keeps its centre) and each centre's squared shift.
__global__ __launch_bounds__(kBlock) void k_lloyd_update(const double* __restrict__ mom, int k, double* __restrict__ mu,
                                                         double* __restrict__ shift) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= k) return;
    const double cnt = mom[(int64_t)j * kMom];
    double sh = 0.0;
    if (cnt > 0.0) {
        for (int d = 0; d < 3; ++d) {
            const double c = mom[(int64_t)j * kMom + 1 + d] / cnt;
            const double e = c - mu[3 * j + d];
            sh += e * e;
            mu[3 * j + d] = c;
        }
    }
    shift[j] = sh;
}

// ---- EM ---------------------------------------------------------------------------------------------------------------
// Per point: normaliser lse_i = log sum_k exp(log p(i, k)); per workgroup the sum of its normalisers.
__global__ __launch_bounds__(kBlock) void k_normaliser(const double4* __restrict__ xs, int64_t n,
                                                       const double* __restrict__ rec, int k, double* __restrict__ lse,
                                                       double* __restrict__ qpart) {
    __shared__ double red[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double out = 0.0;
    if (i < n) {
        const double4 p = xs[i];
        double m = -INFINITY;
        for (int j = 0; j < k; ++j) {
            const double* r = rec + (int64_t)j * kRec;
            const double dx = p.x - r[0], dy = p.y - r[1], dz = p.z - r[2];
            m = fmax(m, fma(r[3], dx * dx + dy * dy + dz * dz, r[4]));
        }
        double sum = 0.0;
        for (int j = 0; j < k; ++j) {
            const double* r = rec + (int64_t)j * kRec;
            const double dx = p.x - r[0], dy = p.y - r[1], dz = p.z - r[2];
            sum += exp(fma(r[3], dx * dx + dy * dy + dz * dz, r[4]) - m);
        }
        out = m + log(sum);
        lse[i] = out;
    }
    red[threadIdx.x] = out;
    block_tree_sum<kBlock>(red);
    if (threadIdx.x == 0) qpart[blockIdx.x] = red[0];
}

// Moments of one chunk of points for kCompBlock components: thread = component, points staged through LDS and walked
// in order.  ONE_HOT: resp = (label == component) instead of exp(log p - lse).  part[(chunk * kMom + v) * k + comp].
template <bool ONE_HOT>
__global__ __launch_bounds__(kCompBlock) void k_moments(const double4* __restrict__ xs, int64_t n, int chunk,
                                                        const double* __restrict__ rec, const double* __restrict__ lse,
                                                        const int* __restrict__ labels, int k,
                                                        double* __restrict__ part) {
    __shared__ double4 pts[kCompBlock];
    __shared__ double aux[kCompBlock];  // lse, or the label as a double
    const int j = blockIdx.y * kCompBlock + threadIdx.x;
    const bool live = j < k;
    double mx = 0.0, my = 0.0, mz = 0.0, a = 0.0, b = 0.0;
    if (live && !ONE_HOT) {
        const double* r = rec + (int64_t)j * kRec;
        mx = r[0]; my = r[1]; mz = r[2]; a = r[3]; b = r[4];
    }
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(lo + (int64_t)chunk, n);
    double s0 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, syy = 0.0, szz = 0.0;
    for (int64_t t0 = lo; t0 < hi; t0 += kCompBlock) {
        const int cnt = (int)min((int64_t)kCompBlock, hi - t0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            pts[threadIdx.x] = xs[t0 + threadIdx.x];
            aux[threadIdx.x] = ONE_HOT ? (double)labels[t0 + threadIdx.x] : lse[t0 + threadIdx.x];
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < cnt; ++q) {
            const double4 p = pts[q];
            double r;
            if (ONE_HOT) {
                r = (aux[q] == (double)j) ? 1.0 : 0.0;
            } else {
                const double dx = p.x - mx, dy = p.y - my, dz = p.z - mz;
                r = exp(fma(a, dx * dx + dy * dy + dz * dz, b) - aux[q]);
            }
            s0 += r;
            sx += r * p.x;
            sy += r * p.y;
            sz += r * p.z;
            sxx += r * (p.x * p.x);
            syy += r * (p.y * p.y);
            szz += r * (p.z * p.z);
        }
    }
    if (!live) return;
    double* o = part + (int64_t)blockIdx.x * kMom * k + j;
    o[0] = s0;
    o[(int64_t)k] = sx;
    o[(int64_t)2 * k] = sy;
    o[(int64_t)3 * k] = sz;
    o[(int64_t)4 * k] = sxx;
    o[(int64_t)5 * k] = syy;
    o[(int64_t)6 * k] = szz;
}

// The chunk partials in chunk order -> mom[comp][kMom]
__global__ __launch_bounds__(kBlock) void k_moments_sum(const double* __restrict__ part, int n_chunks, int k,
                                                        double* __restrict__ mom) {
    const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (id >= (int64_t)k * 7) return;
    const int v = (int)(id / k), j = (int)(id % k);
    double t = 0.0;
    for (int c = 0; c < n_chunks; ++c) t += part[((int64_t)c * kMom + v) * k + j];
    mom[(int64_t)j * kMom + v] = t;
}

// scikit-learn's _estimate_gaussian_parameters for covariance_type = "spherical": nk, means, covariances.
__global__ __launch_bounds__(kBlock) void k_mstep(const double* __restrict__ mom, int k, int dim, double reg_covar,
                                                  double* __restrict__ nk, double* __restrict__ mu,
                                                  double* __restrict__ cov) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= k) return;
    const double* m = mom + (int64_t)j * kMom;
    const double w = m[0] + kTenEps;
    double c = 0.0;
    for (int d = 0; d < 3; ++d) {
        const double mean = m[1 + d] / w;
        mu[3 * j + d] = mean;
        if (d < dim) c += m[4 + d] / w - mean * mean + reg_covar;
    }
    nk[j] = w;
    cov[j] = c / (double)dim;
}

// One workgroup: *out = fixed-order sum of a[0..n)
__global__ __launch_bounds__(kChooseThreads) void k_sum(const double* __restrict__ a, int64_t n, double* __restrict__ out) {
    __shared__ double red[kChooseThreads];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kChooseThreads) t += a[i];
    red[threadIdx.x] = t;
    block_tree_sum<kChooseThreads>(red);
    if (threadIdx.x == 0) out[0] = red[0];
}

// weights = nk / (sum nk, or the number of points for the parameters scikit-learn starts from) and the records.
__global__ __launch_bounds__(kBlock) void k_records(const double* __restrict__ nk, const double* __restrict__ total,
                                                    double n_points, int mode, const double* __restrict__ mu,
                                                    const double* __restrict__ cov, int k, int dim,
                                                    double* __restrict__ w, double* __restrict__ rec) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= k) return;
    const double wj = nk[j] / (mode == kFinInit ? n_points : total[0]);
    w[j] = wj;
    const double c = 1.0 / sqrt(cov[j]);  // precisions_cholesky_
    double* r = rec + (int64_t)j * kRec;
    r[0] = mu[3 * j];
    r[1] = mu[3 * j + 1];
    r[2] = mu[3 * j + 2];
    r[3] = -0.5 * (c * c);
    r[4] = log(wj) + (double)dim * log(c) - 0.5 * (double)dim * kLog2Pi;
}

// Records from explicit parameters (weights_init, means_init, precisions_init): c = sqrt(precision).
__global__ __launch_bounds__(kBlock) void k_records_explicit(const double* __restrict__ w, const double* __restrict__ mu,
                                                             const double* __restrict__ prec, int k, int dim,
                                                             double* __restrict__ rec) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= k) return;
    const double c = sqrt(prec[j]);
    double* r = rec + (int64_t)j * kRec;
    r[0] = mu[3 * j];
    r[1] = mu[3 * j + 1];
    r[2] = mu[3 * j + 2];
    r[3] = -0.5 * (c * c);
    r[4] = log(w[j]) + (double)dim * log(c) - 0.5 * (double)dim * kLog2Pi;
}

}  // namespace

struct prg_gmmfit {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    int dim = 0;
    int k = 0;            // components of the current parameters / centres
    bool have_centers = false, have_labels = false, have_params = false, have_cov = false;
    // the points group (dev_buf.h: reset_group), sized by n: all there or none, and n, dim say which
    prg::DevBuf<double4> xs;
    prg::DevBuf<double> lse, mind2, qpart, seed_part, seed_pre;
    prg::DevBuf<int> labels;
    // the component group, sized together: the capacity in components is w.cap, that of the moment partials part.cap
    prg::DevBuf<double> w, mu, cov, nk, rec, mom, shift, part, unif;
    prg::DevBuf<int> centers, cand;
    prg::DevBuf<double> scal;  // [0] lower-bound sum, [1] sum nk, [2] centre shift; allocated once, as is n_changed
    prg::DevBuf<int> n_changed;
};

namespace {

// points per chunk of the moment sweep: a multiple of kCompBlock, at most kMaxMomChunks chunks
int mom_chunk(int64_t n) {
    const int64_t c = prg::round_up(prg::ceil_div(n, kMaxMomChunks), kCompBlock);
    return (int)std::max<int64_t>(c, 2 * kCompBlock);
}

int ensure_comps(prg_gmmfit* h, int k) {
    const int64_t n_chunks = prg::ceil_div(h->n, mom_chunk(h->n));
    const int64_t need = n_chunks * kMom * (int64_t)k;
    if (k <= h->w.cap && need <= h->part.cap) return PRG_OK;
    PRG_HIP(hipStreamSynchronize(h->stream));
    // what the group held goes, whether its successor arrives or not - and with it the labels' use: the moments of the labels
    // are written into this group (both callers drop the labels on success as well)
    h->have_centers = h->have_labels = h->have_params = h->have_cov = false;
    h->k = 0;
    const int64_t kk = k;
    PRG_HIP(prg::reset_group(h->w, kk, h->mu, kk * 3, h->cov, kk, h->nk, kk, h->rec, kk * kRec, h->mom, kk * kMom, h->shift, kk,
                             h->part, need, h->unif, kk * kMaxTrials, h->centers, kk, h->cand, kMaxTrials));
    return PRG_OK;
}

// label (ONE_HOT) or responsibility moments of all components -> h->mom.p
template <bool ONE_HOT>
int moments(prg_gmmfit* h) {
    const int chunk = mom_chunk(h->n);
    const int n_chunks = (int)prg::ceil_div(h->n, chunk);
    const dim3 grid((unsigned)n_chunks, (unsigned)prg::ceil_div(h->k, kCompBlock));
    k_moments<ONE_HOT><<<grid, kCompBlock, 0, h->stream>>>(h->xs.p, h->n, chunk, h->rec.p, h->lse.p, h->labels.p, h->k, h->part.p);
    PRG_HIP(hipGetLastError());
    k_moments_sum<<<(unsigned)prg::ceil_div((int64_t)h->k * 7, kBlock), kBlock, 0, h->stream>>>(h->part.p, n_chunks, h->k,
                                                                                              h->mom.p);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

// M-step from h->mom.p: parameters and records
int mstep(prg_gmmfit* h, double reg_covar, int mode) {
    const unsigned kb = (unsigned)prg::ceil_div(h->k, kBlock);
    k_mstep<<<kb, kBlock, 0, h->stream>>>(h->mom.p, h->k, h->dim, reg_covar, h->nk.p, h->mu.p, h->cov.p);
    PRG_HIP(hipGetLastError());
    k_sum<<<1, kChooseThreads, 0, h->stream>>>(h->nk.p, h->k, h->scal.p + 1);
    PRG_HIP(hipGetLastError());
    k_records<<<kb, kBlock, 0, h->stream>>>(h->nk.p, h->scal.p + 1, (double)h->n, mode, h->mu.p, h->cov.p, h->k, h->dim, h->w.p,
                                            h->rec.p);
    PRG_HIP(hipGetLastError());
    h->have_params = h->have_cov = true;
    return PRG_OK;
}

int check_k(prg_gmmfit* h, int k, const char* who) {
    PRG_REQUIRE(h->xs.p != nullptr, PRG_ERR_STATE, "%s: no data (prg_gmmfit_set_data first)", who);
    PRG_REQUIRE(k >= 1, PRG_ERR_INVALID, "%s: need at least one component", who);
    PRG_REQUIRE((int64_t)k <= h->n, PRG_ERR_INVALID, "%s: %d components for %lld points (need n_components <= n_samples)",
                who, k, (long long)h->n);
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_gmmfit_create(prg_gmmfit** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_gmmfit_destroy(prg_gmmfit* h) {
    return prg::destroy_handle(h);
}

int prg_gmmfit_set_data(prg_gmmfit* h, const double* data_hd, int64_t n, int dim) {
    PRG_REQUIRE(h && data_hd, PRG_ERR_INVALID, "prg_gmmfit_set_data: NULL argument");
    PRG_REQUIRE(dim == 2 || dim == 3, PRG_ERR_INVALID, "prg_gmmfit_set_data: dim must be 2 or 3, got %d", dim);
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_gmmfit_set_data: need 1 <= n < 2^31 points");
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->n = 0;
    h->dim = 0;
    h->k = 0;
    h->have_centers = h->have_labels = h->have_params = h->have_cov = false;
    prg::release_all(h->w, h->mu, h->cov, h->nk, h->rec, h->mom, h->shift, h->part, h->unif, h->centers, h->cand);
    const int64_t nb = prg::ceil_div(n, kBlock);
    hipError_t e = prg::reset_group(h->xs, n, h->lse, n, h->mind2, n, h->labels, n, h->qpart, nb, h->seed_part, nb * kMaxTrials,
                                    h->seed_pre, nb);
    if (e == hipSuccess) e = h->scal.ensure(4, 4);
    if (e == hipSuccess) e = h->n_changed.ensure(1, 1);
    // padded layout (x, y, z or 0, 0): 2-D clouds run through the same kernels with z = 0 on both sides
    std::vector<double> raw, pad;
    const int st = e == hipSuccess ? prg::load_cloud3(data_hd, n, dim, nullptr, raw, pad, nullptr, nullptr) : PRG_OK;
    if (e == hipSuccess && st == PRG_OK)
        e = hipMemcpyAsync(h->xs.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || st != PRG_OK)  // no half-built cloud: the handle is back to "no data"
        prg::release_all(h->xs, h->lse, h->mind2, h->labels, h->qpart, h->seed_part, h->seed_pre);
    PRG_TRY(st);
    PRG_HIP(e);
    h->n = n;
    h->dim = dim;
    return PRG_OK;
}

int prg_gmmfit_seed(prg_gmmfit* h, int k, const double* uniforms_host, int n_trials) {
    PRG_REQUIRE(h && uniforms_host, PRG_ERR_INVALID, "prg_gmmfit_seed: NULL argument");
    PRG_TRY(check_k(h, k, "prg_gmmfit_seed"));
    PRG_REQUIRE(n_trials >= 1 && n_trials <= kMaxTrials, PRG_ERR_INVALID, "prg_gmmfit_seed: n_trials %d not in [1, %d]",
                n_trials, kMaxTrials);
    for (int64_t i = 0; i < (int64_t)k * n_trials; ++i)
        PRG_REQUIRE(uniforms_host[i] >= 0.0 && uniforms_host[i] < 1.0, PRG_ERR_INVALID,
                    "prg_gmmfit_seed: uniforms must lie in [0, 1)");
    PRG_ENTER(h->device);
    PRG_TRY(ensure_comps(h, k));
    h->k = k;
    const int64_t n = h->n;
    const unsigned nb = (unsigned)prg::ceil_div(n, kBlock);
    // the first centre is uniform over the points
    const int first = (int)std::min<int64_t>((int64_t)(uniforms_host[0] * (double)n), n - 1);
    PRG_HIP(hipMemcpyAsync(h->centers.p, &first, sizeof(int), hipMemcpyHostToDevice, h->stream));
    PRG_HIP(hipMemcpyAsync(h->unif.p, uniforms_host, (size_t)k * n_trials * sizeof(double), hipMemcpyHostToDevice,
                           h->stream));
    k_fill<<<nb, kBlock, 0, h->stream>>>(h->mind2.p, n, INFINITY);
    PRG_HIP(hipGetLastError());
    for (int s = 0; s < k; ++s) {
        const int ncand = s == 0 ? 0 : n_trials;
        k_seed_sweep<<<nb, kBlock, 0, h->stream>>>(h->xs.p, n, h->centers.p, s == 0 ? 0 : s - 1, h->cand.p, ncand, h->mind2.p,
                                                   h->seed_part.p);
        PRG_HIP(hipGetLastError());
        k_seed_choose<<<1, kChooseThreads, 0, h->stream>>>(h->xs.p, n, h->mind2.p, h->seed_part.p, (int)nb, ncand, h->cand.p,
                                                           h->centers.p, s, k, h->unif.p, n_trials, h->seed_pre.p);
        PRG_HIP(hipGetLastError());
    }
    k_gather_centers<<<(unsigned)prg::ceil_div(k, kBlock), kBlock, 0, h->stream>>>(h->xs.p, h->centers.p, k, h->mu.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));  // uniforms_host and `first` may be released
    h->have_centers = true;
    h->have_labels = h->have_params = h->have_cov = false;
    return PRG_OK;
}

int prg_gmmfit_get_seeds(prg_gmmfit* h, int* index_host) {
    PRG_REQUIRE(h && index_host, PRG_ERR_INVALID, "prg_gmmfit_get_seeds: NULL argument");
    PRG_REQUIRE(h->have_centers && h->centers.p, PRG_ERR_STATE, "prg_gmmfit_get_seeds: prg_gmmfit_seed first");
    PRG_ENTER(h->device);
    return prg::copy_out(index_host, h->centers, h->k, h->stream);
}

int prg_gmmfit_lloyd(prg_gmmfit* h, int max_iter, double tol, int* n_iter_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_gmmfit_lloyd: NULL argument");
    PRG_REQUIRE(h->have_centers, PRG_ERR_STATE, "prg_gmmfit_lloyd: no centres (prg_gmmfit_seed first)");
    PRG_REQUIRE(max_iter >= 1, PRG_ERR_INVALID, "prg_gmmfit_lloyd: max_iter must be >= 1");
    PRG_ENTER(h->device);
    const int64_t n = h->n;
    const unsigned nb = (unsigned)prg::ceil_div(n, kBlock), kb = (unsigned)prg::ceil_div(h->k, kBlock);
    PRG_HIP(hipMemsetAsync(h->labels.p, 0xFF, (size_t)n * sizeof(int), h->stream));  // -1: every label changes first
    bool strict = false;
    int it = 0;
    while (it < max_iter) {
        ++it;
        PRG_HIP(hipMemsetAsync(h->n_changed.p, 0, sizeof(int), h->stream));
        k_assign<<<nb, kBlock, 0, h->stream>>>(h->xs.p, n, h->mu.p, h->k, h->labels.p, h->n_changed.p);
        PRG_HIP(hipGetLastError());
        PRG_TRY(moments<true>(h));
        k_lloyd_update<<<kb, kBlock, 0, h->stream>>>(h->mom.p, h->k, h->mu.p, h->shift.p);
        PRG_HIP(hipGetLastError());
        k_sum<<<1, kChooseThreads, 0, h->stream>>>(h->shift.p, h->k, h->scal.p + 2);
        PRG_HIP(hipGetLastError());
        int changed = 0;
        double shift = 0.0;
        PRG_HIP(hipMemcpyAsync(&changed, h->n_changed.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        PRG_HIP(hipMemcpyAsync(&shift, h->scal.p + 2, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        PRG_HIP(hipStreamSynchronize(h->stream));
        if (changed == 0) {
            strict = true;
            break;
        }
        if (shift <= tol) break;
    }
    if (!strict) {  // labels of the final centres
        PRG_HIP(hipMemsetAsync(h->n_changed.p, 0, sizeof(int), h->stream));
        k_assign<<<nb, kBlock, 0, h->stream>>>(h->xs.p, n, h->mu.p, h->k, h->labels.p, h->n_changed.p);
        PRG_HIP(hipGetLastError());
        PRG_HIP(hipStreamSynchronize(h->stream));
    }
    if (n_iter_host) *n_iter_host = it;
    h->have_labels = true;
    return PRG_OK;
}

int prg_gmmfit_init_from_labels(prg_gmmfit* h, double reg_covar) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_gmmfit_init_from_labels: NULL argument");
    PRG_REQUIRE(h->have_labels, PRG_ERR_STATE, "prg_gmmfit_init_from_labels: no labels (prg_gmmfit_lloyd first)");
    PRG_REQUIRE(reg_covar >= 0.0, PRG_ERR_INVALID, "prg_gmmfit_init_from_labels: reg_covar must be >= 0");
    PRG_ENTER(h->device);
    PRG_TRY(moments<true>(h));
    PRG_TRY(mstep(h, reg_covar, kFinInit));
    PRG_HIP(hipStreamSynchronize(h->stream));
    return PRG_OK;
}

int prg_gmmfit_set_params(prg_gmmfit* h, int k, const double* weights_host, const double* means_host,
                          const double* precisions_host) {
    PRG_REQUIRE(h && weights_host && means_host && precisions_host, PRG_ERR_INVALID,
                "prg_gmmfit_set_params: NULL argument");
    PRG_TRY(check_k(h, k, "prg_gmmfit_set_params"));
    for (int j = 0; j < k; ++j)
        PRG_REQUIRE(precisions_host[j] > 0.0 && weights_host[j] >= 0.0, PRG_ERR_INVALID,
                    "prg_gmmfit_set_params: component %d needs precision > 0 and weight >= 0", j);
    PRG_ENTER(h->device);
    PRG_TRY(ensure_comps(h, k));
    h->k = k;
    std::vector<double> mu((size_t)k * 3, 0.0);
    for (int j = 0; j < k; ++j)
        for (int d = 0; d < h->dim; ++d) mu[(size_t)j * 3 + d] = means_host[(size_t)j * h->dim + d];
    PRG_HIP(hipMemcpyAsync(h->w.p, weights_host, (size_t)k * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PRG_HIP(hipMemcpyAsync(h->mu.p, mu.data(), mu.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PRG_HIP(hipMemcpyAsync(h->nk.p, precisions_host, (size_t)k * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_records_explicit<<<(unsigned)prg::ceil_div(k, kBlock), kBlock, 0, h->stream>>>(h->w.p, h->mu.p, h->nk.p, k, h->dim,
                                                                                    h->rec.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_params = true;
    h->have_cov = h->have_centers = h->have_labels = false;
    return PRG_OK;
}

int prg_gmmfit_em(prg_gmmfit* h, double tol, int max_iter, double reg_covar, int* n_iter_host, int* converged_host,
                  double* lower_bounds_host) {
    PRG_REQUIRE(h && n_iter_host && converged_host, PRG_ERR_INVALID, "prg_gmmfit_em: NULL argument");
    PRG_REQUIRE(h->have_params, PRG_ERR_STATE,
                "prg_gmmfit_em: no parameters (prg_gmmfit_set_params or prg_gmmfit_init_from_labels first)");
    PRG_REQUIRE(max_iter >= 1, PRG_ERR_INVALID, "prg_gmmfit_em: max_iter must be >= 1");
    PRG_REQUIRE(reg_covar >= 0.0, PRG_ERR_INVALID, "prg_gmmfit_em: reg_covar must be >= 0");
    PRG_ENTER(h->device);
    const int64_t n = h->n;
    const unsigned nb = (unsigned)prg::ceil_div(n, kBlock);
    double prev = -std::numeric_limits<double>::infinity();
    int it = 0, conv = 0;
    while (it < max_iter) {
        ++it;
        k_normaliser<<<nb, kBlock, 0, h->stream>>>(h->xs.p, n, h->rec.p, h->k, h->lse.p, h->qpart.p);
        PRG_HIP(hipGetLastError());
        k_sum<<<1, kChooseThreads, 0, h->stream>>>(h->qpart.p, (int64_t)nb, h->scal.p);
        PRG_HIP(hipGetLastError());
        double q = 0.0;
        PRG_HIP(hipMemcpyAsync(&q, h->scal.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        PRG_TRY(moments<false>(h));
        PRG_TRY(mstep(h, reg_covar, kFinNormalise));
        PRG_HIP(hipStreamSynchronize(h->stream));
        const double lb = q / (double)n;
        if (lower_bounds_host) lower_bounds_host[it - 1] = lb;
        if (fabs(lb - prev) < tol) {
            conv = 1;
            break;
        }
        prev = lb;
    }
    *n_iter_host = it;
    *converged_host = conv;
    return PRG_OK;
}

int prg_gmmfit_get_params(prg_gmmfit* h, double* weights_host, double* means_host, double* covariances_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_gmmfit_get_params: NULL argument");
    PRG_REQUIRE(h->have_params || h->have_centers, PRG_ERR_STATE, "prg_gmmfit_get_params: nothing fitted yet");
    PRG_REQUIRE((!weights_host && !covariances_host) || h->have_cov, PRG_ERR_STATE,
                "prg_gmmfit_get_params: weights and covariances exist after an M-step only");
    PRG_ENTER(h->device);
    const int k = h->k;
    std::vector<double> mu((size_t)k * 3);
    PRG_TRY(prg::copy_out(weights_host, h->w, k, h->stream));
    PRG_TRY(prg::copy_out(covariances_host, h->cov, k, h->stream));
    PRG_TRY(prg::copy_out(mu.data(), h->mu, k * 3, h->stream));
    if (means_host)
        for (int j = 0; j < k; ++j)
            for (int d = 0; d < h->dim; ++d) means_host[(size_t)j * h->dim + d] = mu[(size_t)j * 3 + d];
    return PRG_OK;
}

}  // extern "C"
