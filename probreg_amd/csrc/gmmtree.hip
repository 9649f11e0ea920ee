// GMMTree (Eckart et al., ECCV 2018 "HGMR"; reference probreg/cc/gmmtree.{h,cc}): hierarchical 8-ary GMM build and the
// registration E-step, everything in fp64 (the reference's native code is float, cc/types.h:5).
//
// Node layout (device, 10 doubles): pi, mu (3), Sigma (xx, xy, xz, yy, yz, zz).  Per node precompute (12 doubles):
//   [0] pi * c           c = 1 / (sqrt(det) (2 pi)^1.5), 0 when det < 1e-15          (gaussianPdf gmmtree.cc:11-18)
//   [1] the same, 0 when pi < 1e-15                                                   (logLikelihood :25)
//   [2..4] mu  [5..10] Sigma^-1 (xx, xy, xz, yy, yz, zz; 0 when det < 1e-15)  [11] complexity (:35-40)
// Tree indices as the reference (:42-44): level(l) = 8 (8^l - 1) / 7, children of j are (j + 1) 8 ... + 7.
//
// Determinism: no floating-point atomics.  Every sum over points is reduced in a fixed order: the points are ordered by
// the node they feed (a stable radix sort), each node's run of points is cut into fixed chunks of kChunk, a workgroup
// reduces one chunk (per-thread strided sums, wave butterflies, waves in order) and one pass per node adds its chunk
// partials in chunk order.  The chunk table comes from the sorted keys on the device (k_seg_table), so nothing but the
// build's log-likelihood (one double per EM iteration) and the registration moments cross to the host.
#include <math.h>
#include <stdlib.h>

#include <new>
#include <vector>

#include "cell_grid.h"
#include "dev_buf.h"
#include "lattice_sort.h"
#include "prg_common.h"

namespace {

constexpr int kNodeD = 10;   // doubles per node
constexpr int kPreD = 12;    // doubles per node precompute
constexpr int kBlock = 256;
constexpr int kChunk = 2048; // points per reduction chunk
constexpr int kSegThreads = 1024;
constexpr double kEps = 1.0e-15;                    // gmmtree.cc:9
constexpr double kInvTwoPi15 = 0.063493635934240969; // (2 pi)^-1.5

inline int64_t level_begin(int l) {  // gmmtree.cc:44
    int64_t p = 1;
    for (int i = 0; i < l; ++i) p *= 8;
    return 8 * (p - 1) / 7;
}
inline int64_t pow8(int l) {
    int64_t p = 1;
    for (int i = 0; i < l; ++i) p *= 8;
    return p;
}

// Eigenvalues of a symmetric 3 x 3 matrix by cyclic Jacobi rotations (scalars only: no arrays, no scratch).
__device__ inline void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq) {
    if (apq == 0.0) return;
    const double tau = (aqq - app) / (2.0 * apq);
    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    app -= t * apq;
    aqq += t * apq;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
}

// complexity(Sigma) = lambda_min / sum(lambda)   (gmmtree.cc:35-40)
__device__ inline double sym3_complexity(double a00, double a01, double a02, double a11, double a12, double a22) {
    for (int sweep = 0; sweep < 16; ++sweep) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        if (off <= 1e-300 || off <= 1e-18 * (fabs(a00) + fabs(a11) + fabs(a22))) break;
        jacobi_rot(a00, a11, a01, a02, a12);  // plane (0,1), r = 2
        jacobi_rot(a00, a22, a02, a01, a12);  // plane (0,2), r = 1: a_r0 = a01, a_r2 = a12
        jacobi_rot(a11, a22, a12, a01, a02);  // plane (1,2), r = 0: a_r1 = a01, a_r2 = a02
    }
    const double lmin = fmin(a00, fmin(a11, a22));
    return lmin / (a00 + a11 + a22);
}

__device__ inline void node_precompute(const double* __restrict__ nd, double* __restrict__ pre) {
    const double pi = nd[0];
    const double sxx = nd[4], sxy = nd[5], sxz = nd[6], syy = nd[7], syz = nd[8], szz = nd[9];
    const double c00 = syy * szz - syz * syz, c01 = sxz * syz - sxy * szz, c02 = sxy * syz - sxz * syy;
    const double det = sxx * c00 + sxy * c01 + sxz * c02;
    const bool live = det >= kEps;  // gmmtree.cc:14: `if (det < eps) return 0`
    const double inv = live ? 1.0 / det : 0.0;
    const double pic = live ? pi * kInvTwoPi15 / sqrt(det) : 0.0;
    pre[0] = pic;
    pre[1] = (pi < kEps) ? 0.0 : pic;
    pre[2] = nd[1];
    pre[3] = nd[2];
    pre[4] = nd[3];
    pre[5] = c00 * inv;
    pre[6] = c01 * inv;
    pre[7] = c02 * inv;
    pre[8] = (sxx * szz - sxz * sxz) * inv;
    pre[9] = (sxy * sxz - sxx * syz) * inv;
    pre[10] = (sxx * syy - sxy * sxy) * inv;
    pre[11] = sym3_complexity(sxx, sxy, sxz, syy, syz, szz);
}

// pi_j c_j exp(-1/2 d^T Sigma_j^-1 d) from a precompute record (w = pre[0] or pre[1])
__device__ inline double weighted_pdf(const double* __restrict__ pr, double w, double x, double y, double z) {
    const double dx = x - pr[2], dy = y - pr[3], dz = z - pr[4];
    const double q = pr[5] * dx * dx + pr[8] * dy * dy + pr[10] * dz * dz +
                     2.0 * (pr[6] * dx * dy + pr[7] * dx * dz + pr[9] * dy * dz);
    return w == 0.0 ? 0.0 : w * exp(-0.5 * q);
}

__global__ __launch_bounds__(kBlock) void k_gmm_precompute(const double* __restrict__ nodes, double* __restrict__ pre,
                                                           int64_t j0, int64_t j1) {
    const int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= j1) return;
    node_precompute(nodes + j * kNodeD, pre + j * kPreD);
}

// Segment / chunk table of n sorted keys in [0, n_seg): seg_start[s] = first position with key >= s (seg_start[n_seg] =
// n), seg_choff[s] = first chunk of segment s (seg_choff[n_seg] = number of chunks).  One workgroup.
__global__ __launch_bounds__(kSegThreads) void k_seg_table(const unsigned* __restrict__ keys, int64_t n, int n_seg,
                                                           int64_t* __restrict__ seg_start, int* __restrict__ seg_choff) {
    __shared__ int sums[kSegThreads];
    const int t = threadIdx.x;
    const int per = (n_seg + kSegThreads - 1) / kSegThreads;
    const int s0 = min(t * per, n_seg), s1 = min(s0 + per, n_seg);
    auto lower = [&](int64_t s) {
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)keys[mid] < s) lo = mid + 1; else hi = mid;
        }
        return lo;
    };
    int local = 0;
    int64_t prev = lower(s0);
    for (int s = s0; s < s1; ++s) {
        const int64_t nxt = lower(s + 1);
        seg_start[s] = prev;
        local += (int)((nxt - prev + kChunk - 1) / kChunk);
        prev = nxt;
    }
    sums[t] = local;
    __syncthreads();
    for (int o = 1; o < kSegThreads; o <<= 1) {  // inclusive Hillis-Steele scan (integers: exact)
        const int v = (t >= o) ? sums[t - o] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    int off = sums[t] - local;
    prev = (s0 < s1) ? seg_start[s0] : 0;
    for (int s = s0; s < s1; ++s) {
        const int64_t nxt = (s + 1 < s1) ? seg_start[s + 1] : lower(s + 1);
        seg_choff[s] = off;
        off += (int)((nxt - prev + kChunk - 1) / kChunk);
        prev = nxt;
    }
    if (t == kSegThreads - 1) {
        seg_choff[n_seg] = sums[t];
        seg_start[n_seg] = n;
    }
}

// Which segment / point range chunk b covers (false: b is past the last chunk).
__device__ inline bool chunk_range(const int64_t* __restrict__ seg_start, const int* __restrict__ seg_choff, int n_seg,
                                   int b, int* seg, int64_t* lo, int64_t* hi) {
    if (b >= seg_choff[n_seg]) return false;
    int l = 0, h = n_seg + 1;  // upper_bound(seg_choff, b) - 1: the non-empty segment whose chunks contain b
    while (l < h) {
        const int mid = (l + h) >> 1;
        if (seg_choff[mid] <= b) l = mid + 1; else h = mid;
    }
    const int s = l - 1;
    *seg = s;
    *lo = seg_start[s] + (int64_t)(b - seg_choff[s]) * kChunk;
    *hi = min(*lo + (int64_t)kChunk, seg_start[s + 1]);
    return true;
}

// Fixed-order workgroup sum of NV per-thread values: wave butterflies, then the waves in order.  Thread v < NV of the
// workgroup receives the value v in out[v] (LDS).
template <int NV>
__device__ inline void block_sum(double (&acc)[NV], double* red /* [kBlock / 64][NV] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double a = acc[v];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        acc[v] = a;
    }
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < NV; ++v) red[wave * NV + v] = acc[v];
    }
    __syncthreads();
}

// ---- build: E-step of one level (gmmTreeEstep gmmtree.cc:125-163) -----------------------------------------------------
// Points xs (sorted by parent), one workgroup per chunk: gamma over the 8 children of the chunk's parent, `current`, and
// the chunk's sums of (gamma, gamma x, gamma x x^T) per child -> part[b][80].
__global__ __launch_bounds__(kBlock) void k_build_estep(const double4* __restrict__ xs, const double* __restrict__ pre,
                                                        int64_t lvl0, const int64_t* __restrict__ seg_start,
                                                        const int* __restrict__ seg_choff, int n_seg,
                                                        int* __restrict__ cur, double* __restrict__ part) {
    __shared__ double npre[8 * kPreD];
    __shared__ double red[(kBlock / 64) * 80];
    int s;
    int64_t lo, hi;
    if (!chunk_range(seg_start, seg_choff, n_seg, blockIdx.x, &s, &lo, &hi)) return;
    const int64_t j0 = lvl0 + 8 * (int64_t)s;
    if (threadIdx.x < 8 * kPreD) npre[threadIdx.x] = pre[j0 * kPreD + threadIdx.x];
    __syncthreads();
    double acc[80];
#pragma unroll
    for (int v = 0; v < 80; ++v) acc[v] = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kBlock) {
        const double4 p = xs[i];
        double g[8], den = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            g[c] = weighted_pdf(npre + c * kPreD, npre[c * kPreD], p.x, p.y, p.z);
            den += g[c];
        }
        const double inv = den > kEps ? 1.0 / den : 0.0;
        int best = 0;
        double bg = -1.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            g[c] = den > kEps ? g[c] * inv : 0.0;
            if (g[c] > bg) { bg = g[c]; best = c; }  // first maximum (Eigen maxCoeff)
        }
        cur[i] = (int)(j0 + best);
        const double xx = p.x * p.x, xy = p.x * p.y, xz = p.x * p.z, yy = p.y * p.y, yz = p.y * p.z, zz = p.z * p.z;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            acc[c * 10 + 0] += g[c];
            acc[c * 10 + 1] += g[c] * p.x;
            acc[c * 10 + 2] += g[c] * p.y;
            acc[c * 10 + 3] += g[c] * p.z;
            acc[c * 10 + 4] += g[c] * xx;
            acc[c * 10 + 5] += g[c] * xy;
            acc[c * 10 + 6] += g[c] * xz;
            acc[c * 10 + 7] += g[c] * yy;
            acc[c * 10 + 8] += g[c] * yz;
            acc[c * 10 + 9] += g[c] * zz;
        }
    }
    block_sum<80>(acc, red);
    if (threadIdx.x < 80) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += red[w * 80 + threadIdx.x];
        part[(int64_t)blockIdx.x * 80 + threadIdx.x] = t;
    }
}

// ---- build: M-step of one level (gmmTreeMstep :165-173 / mlEstimator :81-96) + node precompute -----------------------
// One workgroup per parent: its chunk partials in chunk order, then the 8 children.
__global__ __launch_bounds__(128) void k_build_mstep(const double* __restrict__ part, const int* __restrict__ seg_choff,
                                                     int64_t lvl0, double n_points, double lambda_d,
                                                     double* __restrict__ nodes, double* __restrict__ pre) {
    __shared__ double sum[80];
    const int s = blockIdx.x;
    if (threadIdx.x < 80) {
        double t = 0.0;
        for (int b = seg_choff[s]; b < seg_choff[s + 1]; ++b) t += part[(int64_t)b * 80 + threadIdx.x];
        sum[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const int c = threadIdx.x;
        const int64_t j = lvl0 + 8 * (int64_t)s + c;
        const double* m = sum + c * 10;
        double nd[kNodeD];
        nd[0] = m[0] / n_points;
        if (m[0] < lambda_d) {
            nd[0] = 0.0;
            nd[1] = nd[2] = nd[3] = 0.0;
            nd[4] = 1.0; nd[5] = 0.0; nd[6] = 0.0; nd[7] = 1.0; nd[8] = 0.0; nd[9] = 1.0;
        } else {
            const double mx = m[1] / m[0], my = m[2] / m[0], mz = m[3] / m[0];
            nd[1] = mx; nd[2] = my; nd[3] = mz;
            nd[4] = m[4] / m[0] - mx * mx;
            nd[5] = m[5] / m[0] - mx * my;
            nd[6] = m[6] / m[0] - mx * mz;
            nd[7] = m[7] / m[0] - my * my;
            nd[8] = m[8] / m[0] - my * mz;
            nd[9] = m[9] / m[0] - mz * mz;
        }
#pragma unroll
        for (int k = 0; k < kNodeD; ++k) nodes[j * kNodeD + k] = nd[k];
        node_precompute(nd, pre + j * kPreD);
    }
}

// ---- build: log-likelihood over all nodes of a level (logLikelihood :20-33) --------------------------------------------
constexpr int kLlTile = 256;
__global__ __launch_bounds__(kBlock) void k_build_loglik(const double4* __restrict__ xs, int64_t n,
                                                         const double* __restrict__ pre, int64_t j0, int64_t j1,
                                                         double* __restrict__ qpart) {
    __shared__ double tile[kLlTile * kPreD];
    __shared__ double red[kBlock];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double4 p = make_double4(0.0, 0.0, 0.0, 0.0);
    if (i < n) p = xs[i];
    double tmp = 0.0;
    for (int64_t t0 = j0; t0 < j1; t0 += kLlTile) {
        const int cnt = (int)min((int64_t)kLlTile, j1 - t0);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt * kPreD; k += kBlock) tile[k] = pre[t0 * kPreD + k];
        __syncthreads();
        for (int k = 0; k < cnt; ++k) {
            const double* pr = tile + k * kPreD;
            const double w = pr[1];
            if (w == 0.0) continue;  // wave-uniform: dead, degenerate or pi < eps nodes
            tmp += weighted_pdf(pr, w, p.x, p.y, p.z);
        }
    }
    red[threadIdx.x] = (i < n) ? log(fmax(tmp, kEps)) : 0.0;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) qpart[blockIdx.x] = red[0];
}

// Fixed-order sum of nb partials -> *out (one workgroup).
__global__ __launch_bounds__(kBlock) void k_sum_partials(const double* __restrict__ part, int64_t nb,
                                                         double* __restrict__ out) {
    __shared__ double red[kBlock];
    double t = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += kBlock) t += part[b];
    red[threadIdx.x] = t;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// keys of the next level: the local index of `current` in level l (its parent level), values the identity
__global__ __launch_bounds__(kBlock) void k_keys_from_cur(const int* __restrict__ cur, int64_t n, int64_t lvl0,
                                                          unsigned* __restrict__ keys, int* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    keys[i] = (unsigned)(cur[i] - lvl0);
    vals[i] = (int)i;
}

__global__ __launch_bounds__(kBlock) void k_gather4(const double4* __restrict__ in, const int* __restrict__ idx, int64_t n,
                                                    double4* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = in[idx[i]];
}

// ---- registration E-step (gmmTreeRegEstep gmmtree.cc:175-214) ----------------------------------------------------------
// Transform x = s R p + t, descend from the roots to the first argmax child whose complexity <= lambda_c (or a leaf);
// key = that node, g = its normalised gamma, tx = x.
__global__ __launch_bounds__(kBlock) void k_reg_descend(const double* __restrict__ tgt, int64_t n,
                                                        const double* __restrict__ pre, int levels, double r00, double r01,
                                                        double r02, double r10, double r11, double r12, double r20,
                                                        double r21, double r22, double t0, double t1, double t2,
                                                        double lambda_c, unsigned* __restrict__ keys,
                                                        int* __restrict__ vals, double4* __restrict__ txg) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double px = tgt[3 * i], py = tgt[3 * i + 1], pz = tgt[3 * i + 2];
    const double x = (r00 * px + r01 * py + r02 * pz) + t0;
    const double y = (r10 * px + r11 * py + r12 * pz) + t1;
    const double z = (r20 * px + r21 * py + r22 * pz) + t2;
    int64_t search = -1;
    double gsel = 0.0;
    for (int l = 0; l < levels; ++l) {
        const int64_t j0 = (search + 1) * 8;
        double g[8], den = 0.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double* pr = pre + (j0 + c) * kPreD;
            g[c] = weighted_pdf(pr, pr[0], x, y, z);
            den += g[c];
        }
        const double inv = den > kEps ? 1.0 / den : 0.0;
        int best = 0;
        double bg = -1.0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const double gc = den > kEps ? g[c] * inv : 0.0;
            if (gc > bg) { bg = gc; best = c; }
        }
        search = j0 + best;
        gsel = bg;
        if (pre[search * kPreD + 11] <= lambda_c) break;
    }
    keys[i] = (unsigned)search;
    vals[i] = (int)i;
    txg[i] = make_double4(x, y, z, gsel);
}

__global__ __launch_bounds__(kBlock) void k_reg_chunk(const double4* __restrict__ txg, const int* __restrict__ idx,
                                                      const int64_t* __restrict__ seg_start,
                                                      const int* __restrict__ seg_choff, int n_seg,
                                                      double* __restrict__ part) {
    __shared__ double red[(kBlock / 64) * 10];
    int s;
    int64_t lo, hi;
    if (!chunk_range(seg_start, seg_choff, n_seg, blockIdx.x, &s, &lo, &hi)) return;
    double acc[10];
#pragma unroll
    for (int v = 0; v < 10; ++v) acc[v] = 0.0;
    for (int64_t k = lo + threadIdx.x; k < hi; k += kBlock) {
        const double4 p = txg[idx[k]];
        const double g = p.w;
        acc[0] += g;
        acc[1] += g * p.x;
        acc[2] += g * p.y;
        acc[3] += g * p.z;
        acc[4] += g * (p.x * p.x);
        acc[5] += g * (p.x * p.y);
        acc[6] += g * (p.x * p.z);
        acc[7] += g * (p.y * p.y);
        acc[8] += g * (p.y * p.z);
        acc[9] += g * (p.z * p.z);
    }
    block_sum<10>(acc, red);
    if (threadIdx.x < 10) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) t += red[w * 10 + threadIdx.x];
        part[(int64_t)blockIdx.x * 10 + threadIdx.x] = t;
    }
}

// per (node, value): the node's chunk partials in chunk order -> m01[node][4] (m0, m1), m2[node][6]
__global__ __launch_bounds__(kBlock) void k_reg_final(const double* __restrict__ part, const int* __restrict__ seg_choff,
                                                      int n_nodes, double* __restrict__ m01, double* __restrict__ m2) {
    const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (id >= (int64_t)n_nodes * 10) return;
    const int j = (int)(id / 10), v = (int)(id % 10);
    double t = 0.0;
    for (int b = seg_choff[j]; b < seg_choff[j + 1]; ++b) t += part[(int64_t)b * 10 + v];
    if (v < 4) m01[(int64_t)j * 4 + v] = t;
    else m2[(int64_t)j * 6 + v - 4] = t;
}

}  // namespace

struct prg_gmmtree {
    int device = 0;
    hipStream_t stream = nullptr;
    // the tree group (dev_buf.h: reset_group), sized by n_nodes: all four arrays or none; levels, n_nodes say which
    int levels = 0;
    int64_t n_nodes = 0;
    prg::DevBuf<double> nodes;    // n_nodes x 10
    prg::DevBuf<double> pre;      // n_nodes x 12
    prg::DevBuf<double> m01, m2;  // n_nodes x 4, n_nodes x 6
    // target of the registration E-step
    int64_t n_tgt = 0;
    prg::DevBuf<double> tgt;  // n x 3
    // the workspace group (grown on demand, as a whole): keys.cap points, seg_start.cap - 1 segments, part.cap partials
    size_t sort_bytes = 0;
    prg::DevBuf<unsigned> keys, keys2;
    prg::DevBuf<int> vals, vals2, cur, seg_choff;
    prg::DevBuf<int64_t> seg_start;
    prg::DevBuf<double4> xa, xb;
    prg::DevBuf<double> part;
    prg::DevBuf<char> sort_tmp;
    prg::DevBuf<double> q;  // allocated once
};

namespace {

// Workspaces for n points, n_seg segments and partials of `width` doubles per chunk.
int ensure_ws(prg_gmmtree* h, int64_t n, int64_t n_seg, int width) {
    const int64_t max_chunks = prg::ceil_div(n, kChunk) + n_seg;
    if (n <= h->keys.cap && n_seg < h->seg_start.cap && max_chunks * width <= h->part.cap) return PRG_OK;
    PRG_HIP(hipStreamSynchronize(h->stream));
    const int64_t nn = std::max<int64_t>(n, 1), ns = std::max<int64_t>(n_seg, 8 * 585);  // 585 = level(3) / 8 + 1
    const int64_t np = (prg::ceil_div(nn, kChunk) + ns) * 80;
    size_t bytes = 0;
    PRG_TRY(prg::sort_pairs_u32(nullptr, &bytes, nullptr, nullptr, nullptr, nullptr, (unsigned)nn, 32u, h->stream));
    h->sort_bytes = 0;
    PRG_HIP(prg::reset_group(h->keys, nn, h->keys2, nn, h->vals, nn, h->vals2, nn, h->cur, nn, h->xa, nn, h->xb, nn, h->seg_start,
                             ns + 1, h->seg_choff, ns + 1, h->part, np, h->sort_tmp, (int64_t)std::max<size_t>(bytes, 16)));
    h->sort_bytes = bytes;
    return PRG_OK;
}

int alloc_tree(prg_gmmtree* h, int levels) {
    const int64_t n_nodes = level_begin(levels);
    if (h->levels == levels && h->nodes.p) return PRG_OK;
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->levels = 0;
    h->n_nodes = 0;
    PRG_HIP(prg::reset_group(h->nodes, n_nodes * kNodeD, h->pre, n_nodes * kPreD, h->m01, n_nodes * 4, h->m2, n_nodes * 6));
    h->levels = levels;
    h->n_nodes = n_nodes;
    return PRG_OK;
}

int upload_nodes(prg_gmmtree* h, const double* nodes_host) {
    PRG_HIP(hipMemcpyAsync(h->nodes.p, nodes_host, h->n_nodes * kNodeD * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_gmm_precompute<<<(unsigned)prg::ceil_div(h->n_nodes, kBlock), kBlock, 0, h->stream>>>(h->nodes.p, h->pre.p, 0, h->n_nodes);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));  // nodes_host may be released by the caller
    return PRG_OK;
}

int seg_table(prg_gmmtree* h, const unsigned* keys, int64_t n, int n_seg) {
    k_seg_table<<<1, kSegThreads, 0, h->stream>>>(keys, n, n_seg, h->seg_start.p, h->seg_choff.p);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

// initializeNodes (gmmtree.cc:46-73) with explicit leaf indices; leaf Sigma = C + (m - p_k)(m - p_k)^T, C the cloud's
// centred covariance (= sum_i (p_i - p_k)(p_i - p_k)^T / N).
void init_nodes(const double* pts, int64_t n, int levels, const int64_t* idx, std::vector<double>& nodes) {
    const int64_t n_nodes = level_begin(levels);
    nodes.assign(n_nodes * kNodeD, 0.0);
    double m[3] = {0, 0, 0};
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) m[k] += pts[3 * i + k];
    for (int k = 0; k < 3; ++k) m[k] /= (double)n;
    double cv[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const double d0 = pts[3 * i] - m[0], d1 = pts[3 * i + 1] - m[1], d2 = pts[3 * i + 2] - m[2];
        cv[0] += d0 * d0; cv[1] += d0 * d1; cv[2] += d0 * d2; cv[3] += d1 * d1; cv[4] += d1 * d2; cv[5] += d2 * d2;
    }
    for (int k = 0; k < 6; ++k) cv[k] /= (double)n;
    const int64_t lf = level_begin(levels - 1), nl = pow8(levels);
    for (int64_t j = 0; j < nl; ++j) {
        double* nd = nodes.data() + (lf + j) * kNodeD;
        const double* p = pts + 3 * idx[j];
        const double e0 = m[0] - p[0], e1 = m[1] - p[1], e2 = m[2] - p[2];
        nd[0] = 1.0 / 8.0;
        nd[1] = p[0]; nd[2] = p[1]; nd[3] = p[2];
        nd[4] = cv[0] + e0 * e0; nd[5] = cv[1] + e0 * e1; nd[6] = cv[2] + e0 * e2;
        nd[7] = cv[3] + e1 * e1; nd[8] = cv[4] + e1 * e2; nd[9] = cv[5] + e2 * e2;
    }
    for (int l = levels - 2; l >= 0; --l) {  // moment matching of the 8 children (:55-72)
        const int64_t pidx = level_begin(l), cidx = level_begin(l + 1);
        for (int64_t j = 0; j < pow8(l + 1); ++j) {
            double* nd = nodes.data() + (pidx + j) * kNodeD;
            double mu[3] = {0, 0, 0}, s[6] = {0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 8; ++k) {
                const double* c = nodes.data() + (cidx + j * 8 + k) * kNodeD;
                for (int a = 0; a < 3; ++a) mu[a] += c[1 + a];
                s[0] += c[4] + c[1] * c[1]; s[1] += c[5] + c[1] * c[2]; s[2] += c[6] + c[1] * c[3];
                s[3] += c[7] + c[2] * c[2]; s[4] += c[8] + c[2] * c[3]; s[5] += c[9] + c[3] * c[3];
            }
            for (int a = 0; a < 3; ++a) mu[a] /= 8.0;
            for (int a = 0; a < 6; ++a) s[a] /= 8.0;
            nd[0] = 1.0 / 8.0;
            nd[1] = mu[0]; nd[2] = mu[1]; nd[3] = mu[2];
            nd[4] = s[0] - mu[0] * mu[0]; nd[5] = s[1] - mu[0] * mu[1]; nd[6] = s[2] - mu[0] * mu[2];
            nd[7] = s[3] - mu[1] * mu[1]; nd[8] = s[4] - mu[1] * mu[2]; nd[9] = s[5] - mu[2] * mu[2];
        }
    }
}

}  // namespace

extern "C" {

int prg_gmm_create(prg_gmmtree** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_gmm_destroy(prg_gmmtree* h) {
    return prg::destroy_handle(h);
}

int prg_gmm_build(prg_gmmtree* h, const double* points_hd, int64_t n, int tree_level, const int64_t* init_idx_host,
                  double lambda_s, double lambda_d, int max_iter, int* iters_host, double* q_host, double* dq_host) {
    PRG_REQUIRE(h && points_hd && init_idx_host && iters_host, PRG_ERR_INVALID, "prg_gmm_build: NULL argument");
    PRG_REQUIRE(tree_level >= 1 && tree_level <= 4, PRG_ERR_INVALID, "prg_gmm_build: tree_level %d not in [1, 4]",
                tree_level);
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_gmm_build: need 1 <= n < 2^31 points");
    PRG_REQUIRE(max_iter >= 1, PRG_ERR_INVALID, "prg_gmm_build: max_iter must be >= 1");
    const int64_t nl = pow8(tree_level);
    for (int64_t j = 0; j < nl; ++j)
        PRG_REQUIRE(init_idx_host[j] >= 0 && init_idx_host[j] < n, PRG_ERR_INVALID,
                    "prg_gmm_build: init index %lld out of range", (long long)init_idx_host[j]);
    PRG_ENTER(h->device);
    PRG_TRY(alloc_tree(h, tree_level));
    PRG_TRY(ensure_ws(h, n, nl / 8, 80));
    PRG_HIP(h->q.ensure(8, 8));
    // host copy of the points: initialisation (not a hot path) and the padded device layout
    std::vector<double> pts, pad, init;
    PRG_TRY(prg::load_cloud3(points_hd, n, 3, nullptr, pts, pad, nullptr, nullptr));
    PRG_HIP(hipMemcpyAsync(h->xa.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    init_nodes(pts.data(), n, tree_level, init_idx_host, init);
    PRG_TRY(upload_nodes(h, init.data()));

    const unsigned nbl = (unsigned)prg::ceil_div(n, kBlock);
    for (int l = 0; l < tree_level; ++l) {
        const int n_seg = (int)pow8(l);
        const int64_t lvl0 = level_begin(l), lvl1 = level_begin(l + 1);
        if (l == 0) {
            PRG_HIP(hipMemsetAsync(h->keys.p, 0, n * sizeof(unsigned), h->stream));
        } else {
            // order the points by parent (= `current` of the previous level's last E-step, :120); stable
            k_keys_from_cur<<<nbl, kBlock, 0, h->stream>>>(h->cur.p, n, level_begin(l - 1), h->keys2.p, h->vals2.p);
            PRG_HIP(hipGetLastError());
            size_t bytes = h->sort_bytes;
            PRG_TRY(prg::sort_pairs_u32(h->sort_tmp.p, &bytes, h->keys2.p, h->keys.p, h->vals2.p, h->vals.p, (unsigned)n, 3u * l,
                                        h->stream));
            k_gather4<<<nbl, kBlock, 0, h->stream>>>(h->xa.p, h->vals.p, n, h->xb.p);
            PRG_HIP(hipGetLastError());
            h->xa.swap(h->xb);
        }
        PRG_TRY(seg_table(h, h->keys.p, n, n_seg));
        const unsigned max_chunks = (unsigned)(prg::ceil_div(n, kChunk) + n_seg);
        double prev_q = 0.0, q = 0.0;
        int it = 0;
        while (true) {
            ++it;
            k_build_estep<<<max_chunks, kBlock, 0, h->stream>>>(h->xa.p, h->pre.p, lvl0, h->seg_start.p, h->seg_choff.p, n_seg,
                                                                h->cur.p, h->part.p);
            PRG_HIP(hipGetLastError());
            k_build_mstep<<<(unsigned)n_seg, 128, 0, h->stream>>>(h->part.p, h->seg_choff.p, lvl0, (double)n, lambda_d,
                                                                  h->nodes.p, h->pre.p);
            PRG_HIP(hipGetLastError());
            k_build_loglik<<<nbl, kBlock, 0, h->stream>>>(h->xa.p, n, h->pre.p, lvl0, lvl1, h->part.p);
            PRG_HIP(hipGetLastError());
            k_sum_partials<<<1, kBlock, 0, h->stream>>>(h->part.p, (int64_t)nbl, h->q.p);
            PRG_HIP(hipGetLastError());
            PRG_HIP(hipMemcpyAsync(&q, h->q.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
            PRG_HIP(hipStreamSynchronize(h->stream));
            const double dq = fabs(q - prev_q);
            if (dq < lambda_s || it >= max_iter) {  // :116 (the cap is ours: the reference loops until convergence)
                if (dq_host) dq_host[l] = dq;
                break;
            }
            prev_q = q;
        }
        iters_host[l] = it;
        if (q_host) q_host[l] = q;
    }
    return PRG_OK;
}

int prg_gmm_set_nodes(prg_gmmtree* h, const double* nodes_host, int tree_level) {
    PRG_REQUIRE(h && nodes_host, PRG_ERR_INVALID, "prg_gmm_set_nodes: NULL argument");
    PRG_REQUIRE(tree_level >= 1 && tree_level <= 4, PRG_ERR_INVALID, "prg_gmm_set_nodes: tree_level %d not in [1, 4]",
                tree_level);
    PRG_ENTER(h->device);
    PRG_TRY(alloc_tree(h, tree_level));
    return upload_nodes(h, nodes_host);
}

int prg_gmm_get_nodes(prg_gmmtree* h, double* nodes_host) {
    PRG_REQUIRE(h && nodes_host, PRG_ERR_INVALID, "prg_gmm_get_nodes: NULL argument");
    PRG_REQUIRE(h->nodes.p, PRG_ERR_STATE, "prg_gmm_get_nodes: no tree (build or set_nodes first)");
    PRG_ENTER(h->device);
    return prg::copy_out(nodes_host, h->nodes, h->n_nodes * kNodeD, h->stream);
}

int prg_gmm_set_target(prg_gmmtree* h, const double* target_hd, int64_t n) {
    PRG_REQUIRE(h && target_hd, PRG_ERR_INVALID, "prg_gmm_set_target: NULL argument");
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_gmm_set_target: need 1 <= n < 2^31 points");
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->n_tgt = 0;
    hipError_t e = h->tgt.reset(n * 3);
    if (e == hipSuccess) e = hipMemcpyAsync(h->tgt.p, target_hd, (size_t)n * 3 * sizeof(double), hipMemcpyDefault, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) h->tgt.release();  // no target rather than one whose contents never arrived
    PRG_HIP(e);
    h->n_tgt = n;
    return PRG_OK;
}

int prg_gmm_reg_estep(prg_gmmtree* h, const double* rot9, const double* t3, double scale, double lambda_c,
                      double* m01_host, double* m2_host) {
    PRG_REQUIRE(h && rot9 && t3 && m01_host, PRG_ERR_INVALID, "prg_gmm_reg_estep: NULL argument");
    PRG_REQUIRE(h->nodes.p && h->tgt.p, PRG_ERR_STATE, "prg_gmm_reg_estep: need a tree and a target");
    PRG_ENTER(h->device);
    const int64_t n = h->n_tgt;
    const int n_seg = (int)h->n_nodes;
    PRG_TRY(ensure_ws(h, n, n_seg, 80));
    unsigned bits = 1;
    while (((int64_t)1 << bits) < h->n_nodes) ++bits;
    const unsigned nbl = (unsigned)prg::ceil_div(n, kBlock);
    double r[9];
    for (int k = 0; k < 9; ++k) r[k] = scale * rot9[k];
    k_reg_descend<<<nbl, kBlock, 0, h->stream>>>(h->tgt.p, n, h->pre.p, h->levels, r[0], r[1], r[2], r[3], r[4], r[5], r[6],
                                                 r[7], r[8], t3[0], t3[1], t3[2], lambda_c, h->keys2.p, h->vals2.p, h->xb.p);
    PRG_HIP(hipGetLastError());
    size_t bytes = h->sort_bytes;
    PRG_TRY(prg::sort_pairs_u32(h->sort_tmp.p, &bytes, h->keys2.p, h->keys.p, h->vals2.p, h->vals.p, (unsigned)n, bits, h->stream));
    PRG_TRY(seg_table(h, h->keys.p, n, n_seg));
    const unsigned max_chunks = (unsigned)(prg::ceil_div(n, kChunk) + n_seg);
    k_reg_chunk<<<max_chunks, kBlock, 0, h->stream>>>(h->xb.p, h->vals.p, h->seg_start.p, h->seg_choff.p, n_seg, h->part.p);
    PRG_HIP(hipGetLastError());
    k_reg_final<<<(unsigned)prg::ceil_div((int64_t)n_seg * 10, kBlock), kBlock, 0, h->stream>>>(h->part.p, h->seg_choff.p,
                                                                                              n_seg, h->m01.p, h->m2.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(m01_host, h->m01.p, h->n_nodes * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (m2_host)
        PRG_HIP(hipMemcpyAsync(m2_host, h->m2.p, h->n_nodes * 6 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    return PRG_OK;
}

}  // extern "C"
