// FPFH descriptor (Rusu et al. 2009) as the reference gets it from Open3D for `feature_fn` of FilterReg: a hybrid
// (radius + max_nn) neighbour search, PCA normals, the simplified point feature histograms and their 1 / d^2 weighted
// gather.  Everything in fp64; DESIGN.md section 3.9 is the definition with every tie rule.  One stage per entry point:
//
//   grid     the cell grid of cell_grid.h with cell edge = search radius, built anew for every search.
//   search   one wave per query.  The cells that meet [p - r, p + r] (2 to 4 per axis) are dealt to the lanes, keys that
//            repeat (hash collisions) are dropped, then the wave walks the buckets 64 candidates at a time.  Pass 1 counts
//            the candidates.  If they do not fit the list, an MSB-first radix select (8 bits per pass, 256 counters in
//            LDS) over the 96-bit key (bits of d2, point index) finds the key of the last entry that fits - non-negative
//            doubles order as their bit patterns - recomputing d2 in every pass instead of storing candidates, so any
//            number of candidates is handled in constant space.  The last pass compacts the entries at or below that
//            key into LDS, a rank sort puts them into (d2, index) order behind the query itself.
//   normals  one wave per point: the list is rank-sorted by point index into LDS, then mean and centred products are
//            summed in that order (two passes), so equal neighbour sets give bit-identical normals; cyclic Jacobi on
//            the symmetric 3 x 3 covariance.
//   spfh     one wave per point: a lane per neighbour computes the pair feature and its three bins into LDS, then lane
//            b counts bin b over the list; the row is 100 count / (L - 1).  No atomics.
//   fpfh     one wave per point, lane b owns bin b and walks the stored list in list order.
// Two runs on the same input give byte-identical results: the only atomics are integer counters of the radix select.
//
// d2 and every other decision value is computed with separately rounded multiplications and additions (no contraction
// into FMAs), so that a restatement in plain IEEE arithmetic takes the same branches.
#pragma clang fp contract(off)
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <new>
#include <vector>

#include "cell_grid.h"
#include "dev_buf.h"
#include "prg_common.h"
#include "smallest_eigenvector.h"

namespace {

constexpr int kWave = 64;              // every per-point kernel is one wave per workgroup: __syncthreads is wave-local
constexpr int kMaxNN = 512;            // longest neighbour list (LDS of the search, normals and spfh kernels)
constexpr int kBins = 33;              // 3 groups of 11
constexpr double kReach = 1.0 + 1.0e-12;   // the scanned box is a hair wider than r: covers the rounding of d2 <= r * r

using prg::CellGrid;
using prg::cell_key;
using prg::cell_of;
using prg::smallest_eigenvector;

__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The 96-bit sort key (k1 = bits of d2, k0 = point index), 8 bits at a time; s is the bit offset of the digit.
__device__ inline unsigned key_digit(uint64_t k1, unsigned k0, int s) {
    return s >= 32 ? (unsigned)(k1 >> (s - 32)) & 255u : (k0 >> s) & 255u;
}
__device__ inline bool key_prefix_match(uint64_t k1, unsigned k0, uint64_t p1, unsigned p0, int s) {
    if (s >= 32) {
        const int sh = s - 32 + 8;
        return sh >= 64 || (k1 >> sh) == (p1 >> sh);
    }
    return k1 == p1 && (s + 8 >= 32 || (k0 >> (s + 8)) == (p0 >> (s + 8)));
}
__device__ inline bool key_le(uint64_t k1, unsigned k0, uint64_t t1, unsigned t0) {
    return k1 < t1 || (k1 == t1 && k0 <= t0);
}

// Calls f(valid, j, d2) in every lane for every 64 candidates of the buckets (my_b, my_e) of lanes 0 .. ncell - 1;
// valid: a point other than the query within the radius.  All loop bounds are wave-uniform.
template <class F>
__device__ inline void for_candidates(const double4* __restrict__ sp, int my_b, int my_e, int ncell, const double4 p,
                                      int self, double r2, F&& f) {
    const int lane = threadIdx.x;
    for (int c = 0; c < ncell; ++c) {
        const int b = __shfl(my_b, c, 64), e = __shfl(my_e, c, 64);
        for (int t0 = b; t0 < e; t0 += kWave) {
            const int t = t0 + lane;
            bool v = t < e;
            int j = -1;
            double d2 = 0.0;
            if (v) {
                const double4 q = sp[t];
                j = (int)q.w;
                const double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                d2 = dx * dx + dy * dy + dz * dz;
                v = d2 <= r2 && j != self;
            }
            f(v, j, d2);
        }
    }
}

// One wave per query (workgroup q handles the q-th point in cell order).  Row `self` of out_idx / out_d2 (k entries) gets
// the query first, then its neighbours by ascending (d2, index), cut to k; unused entries are (-1, 0).
__global__ __launch_bounds__(kWave) void k_search(const double4* __restrict__ sp, const int2* __restrict__ cells, CellGrid g,
                                                  double r, int k, int* __restrict__ out_idx, double* __restrict__ out_d2,
                                                  int* __restrict__ out_cnt) {
    __shared__ int hist[256];
    __shared__ double l_d2[kMaxNN];
    __shared__ int l_j[kMaxNN];
    const int lane = threadIdx.x;
    const double4 p = sp[blockIdx.x];
    const int self = (int)p.w;
    const double r2 = r * r, reach = r * kReach;

    // the cells that meet [p - reach, p + reach], dealt to the lanes
    const double pc[3] = {p.x, p.y, p.z};
    int c0[3], nc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int lo = cell_of(pc[a] - reach, g.lo[a], g.edge), hi = cell_of(pc[a] + reach, g.lo[a], g.edge);
        lo = min(lo, g.dim[a] - 1);
        hi = min(min(hi, g.dim[a] - 1), lo + 3);
        c0[a] = lo;
        nc[a] = hi - lo + 1;  // 1 .. 4
    }
    const int ncell = nc[0] * nc[1] * nc[2];  // <= 64
    unsigned key = 0;
    if (lane < ncell)
        key = cell_key(c0[0] + lane % nc[0], c0[1] + (lane / nc[0]) % nc[1], c0[2] + lane / (nc[0] * nc[1]), g);
    bool dup = false;  // a bucket is walked once, however many of the cells hash to it
    for (int c = 0; c < ncell; ++c) {
        const unsigned kc = __shfl(key, c, 64);
        dup = dup || (c < lane && kc == key);
    }
    const bool live = lane < ncell && !dup;
    const int2 be = live ? cells[key] : make_int2(0, 0);
    const int my_b = be.x, my_e = be.y;

    int cand = 0;
    for_candidates(sp, my_b, my_e, ncell, p, self, r2, [&](bool v, int, double) { cand += v ? 1 : 0; });
    cand = wave_sum(cand);

    const int need = k - 1;
    uint64_t t1 = ~0ull;  // threshold key: everything at or below it is listed
    unsigned t0 = ~0u;
    if (cand > need && need > 0) {
        uint64_t p1 = 0;
        unsigned p0 = 0;
        int remaining = need;  // entries still to take from the keys that share the prefix
        for (int s = 88; s >= 0; s -= 8) {
#pragma unroll
            for (int q = 0; q < 4; ++q) hist[4 * lane + q] = 0;
            __syncthreads();
            for_candidates(sp, my_b, my_e, ncell, p, self, r2, [&](bool v, int j, double d2) {
                const uint64_t k1 = (uint64_t)__double_as_longlong(d2);
                if (v && key_prefix_match(k1, (unsigned)j, p1, p0, s)) atomicAdd(&hist[key_digit(k1, (unsigned)j, s)], 1);
            });
            __syncthreads();
            const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const int tot = h0 + h1 + h2 + h3;
            int inc = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            const int exc = inc - tot;
            const bool mine = exc < remaining && remaining <= inc;  // exactly one lane
            int bin = 0, below = 0, hb = 0;
            if (mine) {
                if (exc + h0 >= remaining) { bin = 4 * lane; below = exc; hb = h0; }
                else if (exc + h0 + h1 >= remaining) { bin = 4 * lane + 1; below = exc + h0; hb = h1; }
                else if (exc + h0 + h1 + h2 >= remaining) { bin = 4 * lane + 2; below = exc + h0 + h1; hb = h2; }
                else { bin = 4 * lane + 3; below = exc + h0 + h1 + h2; hb = h3; }
            }
            const unsigned long long mm = __ballot(mine);
            const int src = mm ? __ffsll(mm) - 1 : 0;
            bin = __shfl(bin, src, 64);
            below = __shfl(below, src, 64);
            hb = __shfl(hb, src, 64);
            remaining -= below;
            if (s >= 32) p1 |= (uint64_t)bin << (s - 32);
            else p0 |= (unsigned)bin << s;
            if (hb == remaining || s == 0) {  // the whole bin is taken: every lower bit of the threshold is one
                if (s >= 32) { p1 |= (1ull << (s - 32)) - 1ull; p0 = ~0u; }
                else p0 |= (1u << s) - 1u;
                break;
            }
        }
        t1 = p1;
        t0 = p0;
    }

    int m = 0;
    if (need > 0) {
        for_candidates(sp, my_b, my_e, ncell, p, self, r2, [&](bool v, int j, double d2) {
            const bool take = v && key_le((uint64_t)__double_as_longlong(d2), (unsigned)j, t1, t0);
            const unsigned long long mask = __ballot(take);
            const int pos = m + __popcll(mask & ((1ull << lane) - 1ull));
            if (take && pos < kMaxNN) { l_d2[pos] = d2; l_j[pos] = j; }
            m += __popcll(mask);
        });
        m = min(m, need);
    }
    __syncthreads();

    const size_t base = (size_t)self * (size_t)k;
    for (int e = lane; e < m; e += kWave) {
        const double de = l_d2[e];
        const int je = l_j[e];
        int rank = 0;
        for (int f = 0; f < m; ++f) {
            const double df = l_d2[f];
            rank += (df < de || (df == de && l_j[f] < je)) ? 1 : 0;
        }
        out_idx[base + 1 + rank] = je;
        out_d2[base + 1 + rank] = de;
    }
    for (int e = m + 1 + lane; e < k; e += kWave) {
        out_idx[base + e] = -1;
        out_d2[base + e] = 0.0;
    }
    if (lane == 0) {
        out_idx[base] = self;
        out_d2[base] = 0.0;
        out_cnt[self] = m + 1;
    }
}


__global__ __launch_bounds__(kWave) void k_normals(const double4* __restrict__ pts, const int* __restrict__ idx,
                                                   const int* __restrict__ cnt, int k, double* __restrict__ normals) {
    __shared__ int s_idx[kMaxNN];
    __shared__ double s_p[kMaxNN][3];
    const int lane = threadIdx.x;
    const size_t i = blockIdx.x;
    const int L = min(cnt[i], min(k, kMaxNN));
    if (L < 3) {
        if (lane < 3) normals[i * 3 + lane] = lane == 2 ? 1.0 : 0.0;
        return;
    }
    for (int e = lane; e < L; e += kWave) s_idx[e] = idx[i * k + e];
    __syncthreads();
    for (int e = lane; e < L; e += kWave) {  // ascending point index (the indices of a list are distinct)
        const int je = s_idx[e];
        int rank = 0;
        for (int f = 0; f < L; ++f) rank += s_idx[f] < je ? 1 : 0;
        const double4 q = pts[je];
        s_p[rank][0] = q.x;
        s_p[rank][1] = q.y;
        s_p[rank][2] = q.z;
    }
    __syncthreads();
    // every lane runs the same sequential sums (LDS broadcasts); lane 0 stores
    double mx = 0.0, my = 0.0, mz = 0.0;
    for (int e = 0; e < L; ++e) {
        mx += s_p[e][0];
        my += s_p[e][1];
        mz += s_p[e][2];
    }
    const double cntd = (double)L;
    mx /= cntd;
    my /= cntd;
    mz /= cntd;
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = 0; e < L; ++e) {
        const double dx = s_p[e][0] - mx, dy = s_p[e][1] - my, dz = s_p[e][2] - mz;
        c[0] += dx * dx;
        c[1] += dx * dy;
        c[2] += dx * dz;
        c[3] += dy * dy;
        c[4] += dy * dz;
        c[5] += dz * dz;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) c[q] /= cntd;
    double nrm[3];
    smallest_eigenvector(c, nrm);
    if (lane == 0) {
        normals[i * 3 + 0] = nrm[0];
        normals[i * 3 + 1] = nrm[1];
        normals[i * 3 + 2] = nrm[2];
    }
}

__device__ inline int bin11(double x) {  // floor, clamped to the group's 0 .. 10
    const double b = floor(x);
    return !(b > 0.0) ? 0 : (b > 10.0 ? 10 : (int)b);
}

// The three bins of the pair feature of (p1, n1), (p2, n2).
__device__ inline void pair_bins(const double4 p1, const double* n1, const double4 p2, const double* n2, int bins[3]) {
    double f1 = 0.0, f2 = 0.0, f3 = 0.0;
    double dx = p2.x - p1.x, dy = p2.y - p1.y, dz = p2.z - p1.z;
    const double rho = sqrt(dx * dx + dy * dy + dz * dz);
    if (rho != 0.0) {
        const double a1 = (n1[0] * dx + n1[1] * dy + n1[2] * dz) / rho;
        const double a2 = (n2[0] * dx + n2[1] * dy + n2[2] * dz) / rho;
        double ax = n1[0], ay = n1[1], az = n1[2], bx = n2[0], by = n2[1], bz = n2[2];
        if (fabs(a1) < fabs(a2)) {
            ax = n2[0]; ay = n2[1]; az = n2[2];
            bx = n1[0]; by = n1[1]; bz = n1[2];
            dx = -dx; dy = -dy; dz = -dz;
            f3 = -a2;
        } else {
            f3 = a1;
        }
        double vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;  // d x n1
        const double vn = sqrt(vx * vx + vy * vy + vz * vz);
        if (vn != 0.0) {
            vx /= vn; vy /= vn; vz /= vn;
            const double wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;  // n1 x v
            f2 = vx * bx + vy * by + vz * bz;
            f1 = atan2(wx * bx + wy * by + wz * bz, ax * bx + ay * by + az * bz);
        } else {
            f3 = 0.0;
        }
    }
    bins[0] = bin11(11.0 * (f1 + M_PI) / (2.0 * M_PI));
    bins[1] = 11 + bin11(11.0 * (f2 + 1.0) / 2.0);
    bins[2] = 22 + bin11(11.0 * (f3 + 1.0) / 2.0);
}

__global__ __launch_bounds__(kWave) void k_spfh(const double4* __restrict__ pts, const double* __restrict__ normals,
                                                const int* __restrict__ idx, const int* __restrict__ cnt, int k,
                                                double* __restrict__ spfh) {
    __shared__ unsigned char s_bin[3][kMaxNN];
    const int lane = threadIdx.x;
    const size_t i = blockIdx.x;
    const int L = min(cnt[i], min(k, kMaxNN));
    if (L <= 1) {
        if (lane < kBins) spfh[i * kBins + lane] = 0.0;
        return;
    }
    const double4 p1 = pts[i];
    const double n1[3] = {normals[i * 3], normals[i * 3 + 1], normals[i * 3 + 2]};
    for (int e = 1 + lane; e < L; e += kWave) {
        const size_t j = (size_t)idx[i * k + e];
        const double n2[3] = {normals[j * 3], normals[j * 3 + 1], normals[j * 3 + 2]};
        int bins[3];
        pair_bins(p1, n1, pts[j], n2, bins);
        s_bin[0][e] = (unsigned char)bins[0];
        s_bin[1][e] = (unsigned char)bins[1];
        s_bin[2][e] = (unsigned char)bins[2];
    }
    __syncthreads();
    if (lane < kBins) {
        const int grp = lane / 11;
        int count = 0;
        for (int e = 1; e < L; ++e) count += s_bin[grp][e] == lane ? 1 : 0;
        spfh[i * kBins + lane] = 100.0 * (double)count / (double)(L - 1);
    }
}

__global__ __launch_bounds__(kWave) void k_fpfh(const double* __restrict__ spfh, const int* __restrict__ idx,
                                                const double* __restrict__ d2, const int* __restrict__ cnt, int k,
                                                double* __restrict__ fpfh) {
    __shared__ double s_acc[kBins];
    const int lane = threadIdx.x;
    const size_t i = blockIdx.x;
    const int L = min(cnt[i], k);
    double acc = 0.0;
    if (lane < kBins)
        for (int e = 1; e < L; ++e) {
            const double d = d2[i * k + e];
            if (d != 0.0) acc += spfh[(size_t)idx[i * k + e] * kBins + lane] / d;
        }
    if (lane < kBins) s_acc[lane] = acc;
    __syncthreads();
    if (lane < kBins) {
        const int grp = lane / 11;
        double sum = 0.0;
        for (int q = 0; q < 11; ++q) sum += s_acc[grp * 11 + q];
        const double scaled = sum != 0.0 ? acc / sum * 100.0 : 0.0;
        fpfh[i * kBins + lane] = L <= 1 ? 0.0 : scaled + spfh[i * kBins + lane];
    }
}

// one group (dev_buf.h: reset_group): idx and d2 are [n][k], cnt is [n]; k and valid are written once a search has filled them
struct NeighbourLists {
    prg::DevBuf<int> idx;
    prg::DevBuf<double> d2;
    prg::DevBuf<int> cnt;
    int k = 0;
    bool valid = false;
};

}  // namespace

struct prg_fpfh {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;
    prg::DevBuf<double4> pts;  // the cloud group: pts [n], normals [n][3], spfh and fpfh [n][kBins]; n says whether it is there
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    NeighbourLists nb[2];  // 0: normals, 1: features
    prg::DevBuf<double> normals, spfh, fpfh;
    bool have_normals = false, have_spfh = false, have_fpfh = false;
};

namespace {

int run_search(prg_fpfh* h, NeighbourLists& out, double radius, int k) {
    const int64_t n = h->n;
    const unsigned bits = prg::cell_table_bits(n);
    const CellGrid g = prg::make_cell_grid(h->lo, h->hi, radius, bits);
    prg::CellGridScratch s;
    prg::DevBuf<double4> sp;
    prg::DevBuf<int2> cells;
    PRG_TRY(s.size(n, bits));
    PRG_HIP(sp.reset(n));
    PRG_HIP(cells.reset(prg::cell_entries(g)));
    PRG_TRY(prg::build_cell_grid(g, bits, h->pts.p, n, s, sp.p, cells.p, h->stream));
    k_search<<<(unsigned)n, kWave, 0, h->stream>>>(sp.p, cells.p, g, radius, k, out.idx.p, out.d2.p, out.cnt.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));  // the scratch goes away with this scope
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_fpfh_create(prg_fpfh** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_fpfh_destroy(prg_fpfh* h) {
    return prg::destroy_handle(h);
}

int prg_fpfh_max_nn(int* max_nn_host) {
    PRG_REQUIRE(max_nn_host != nullptr, PRG_ERR_INVALID, "prg_fpfh_max_nn: NULL argument");
    *max_nn_host = kMaxNN;
    return PRG_OK;
}

int prg_fpfh_set_data(prg_fpfh* h, const double* points_hd, int64_t n) {
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_fpfh_set_data: NULL argument");
    PRG_REQUIRE(n >= 1 && n <= (int64_t)1 << 30, PRG_ERR_INVALID, "prg_fpfh_set_data: need 1 <= n <= 2^30 points");
    PRG_ENTER(h->device);
    std::vector<double> raw, pad;
    double lo[3], hi[3];
    PRG_TRY(prg::load_cloud3(points_hd, n, 3, "prg_fpfh_set_data: data contains NaN or infinity", raw, pad, lo, hi));
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->n = 0;
    h->have_normals = h->have_spfh = h->have_fpfh = false;
    for (NeighbourLists& l : h->nb) {
        prg::release_all(l.idx, l.d2, l.cnt);
        l.k = 0;
        l.valid = false;
    }
    hipError_t e = prg::reset_group(h->pts, n, h->normals, n * 3, h->spfh, n * kBins, h->fpfh, n * kBins);
    if (e == hipSuccess) e = hipMemcpyAsync(h->pts.p, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) prg::release_all(h->pts, h->normals, h->spfh, h->fpfh);  // no half-built cloud: back to "no data"
    PRG_HIP(e);
    h->n = n;
    for (int a = 0; a < 3; ++a) {
        h->lo[a] = lo[a];
        h->hi[a] = hi[a];
    }
    return PRG_OK;
}

int prg_fpfh_search(prg_fpfh* h, int which, double radius, int max_nn) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fpfh_search: NULL argument");
    PRG_REQUIRE(which == 0 || which == 1, PRG_ERR_INVALID, "prg_fpfh_search: which must be 0 (normals) or 1 (features)");
    PRG_REQUIRE(radius > 0.0 && std::isfinite(radius), PRG_ERR_INVALID, "prg_fpfh_search: radius must be > 0 and finite");
    PRG_REQUIRE(max_nn >= 1 && max_nn <= kMaxNN, PRG_ERR_INVALID, "prg_fpfh_search: max_nn must lie in 1 .. %d, got %d",
                kMaxNN, max_nn);
    PRG_REQUIRE(h->pts.p != nullptr, PRG_ERR_STATE, "prg_fpfh_search: no data (prg_fpfh_set_data first)");
    PRG_ENTER(h->device);
    NeighbourLists& l = h->nb[which];
    PRG_HIP(hipStreamSynchronize(h->stream));
    l.k = 0;
    l.valid = false;
    if (which == 1) h->have_spfh = h->have_fpfh = false;
    const int64_t slots = h->n * max_nn;
    PRG_HIP(prg::reset_group(l.idx, slots, l.d2, slots, l.cnt, h->n));
    const int st = run_search(h, l, radius, max_nn);
    if (st != PRG_OK) {
        prg::release_all(l.idx, l.d2, l.cnt);
        return st;
    }
    l.k = max_nn;
    l.valid = true;
    return PRG_OK;
}

int prg_fpfh_get_neighbours(prg_fpfh* h, int which, int* idx_host, double* d2_host, int* count_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fpfh_get_neighbours: NULL argument");
    PRG_REQUIRE(which == 0 || which == 1, PRG_ERR_INVALID, "prg_fpfh_get_neighbours: which must be 0 or 1");
    const NeighbourLists& l = h->nb[which];
    PRG_REQUIRE(l.valid, PRG_ERR_STATE, "prg_fpfh_get_neighbours: prg_fpfh_search first");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(idx_host, l.idx, h->n * l.k, h->stream));
    PRG_TRY(prg::copy_out(d2_host, l.d2, h->n * l.k, h->stream));
    PRG_TRY(prg::copy_out(count_host, l.cnt, h->n, h->stream));
    return PRG_OK;
}

int prg_fpfh_normals(prg_fpfh* h) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fpfh_normals: NULL argument");
    PRG_REQUIRE(h->nb[0].valid, PRG_ERR_STATE, "prg_fpfh_normals: prg_fpfh_search(0, ...) first");
    PRG_ENTER(h->device);
    k_normals<<<(unsigned)h->n, kWave, 0, h->stream>>>(h->pts.p, h->nb[0].idx.p, h->nb[0].cnt.p, h->nb[0].k, h->normals.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_normals = true;
    h->have_spfh = h->have_fpfh = false;
    return PRG_OK;
}

int prg_fpfh_set_normals(prg_fpfh* h, const double* normals_hd) {
    PRG_REQUIRE(h && normals_hd, PRG_ERR_INVALID, "prg_fpfh_set_normals: NULL argument");
    PRG_REQUIRE(h->pts.p != nullptr, PRG_ERR_STATE, "prg_fpfh_set_normals: no data (prg_fpfh_set_data first)");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_in(h->normals, normals_hd, h->n * 3, h->stream));
    h->have_normals = true;
    h->have_spfh = h->have_fpfh = false;
    return PRG_OK;
}

int prg_fpfh_get_normals(prg_fpfh* h, double* normals_host) {
    PRG_REQUIRE(h && normals_host, PRG_ERR_INVALID, "prg_fpfh_get_normals: NULL argument");
    PRG_REQUIRE(h->have_normals, PRG_ERR_STATE, "prg_fpfh_get_normals: prg_fpfh_normals or prg_fpfh_set_normals first");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(normals_host, h->normals, h->n * 3, h->stream));
    return PRG_OK;
}

int prg_fpfh_spfh(prg_fpfh* h) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fpfh_spfh: NULL argument");
    PRG_REQUIRE(h->nb[1].valid, PRG_ERR_STATE, "prg_fpfh_spfh: prg_fpfh_search(1, ...) first");
    PRG_REQUIRE(h->have_normals, PRG_ERR_STATE, "prg_fpfh_spfh: prg_fpfh_normals or prg_fpfh_set_normals first");
    PRG_ENTER(h->device);
    k_spfh<<<(unsigned)h->n, kWave, 0, h->stream>>>(h->pts.p, h->normals.p, h->nb[1].idx.p, h->nb[1].cnt.p, h->nb[1].k, h->spfh.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_spfh = true;
    h->have_fpfh = false;
    return PRG_OK;
}

int prg_fpfh_get_spfh(prg_fpfh* h, double* spfh_host) {
    PRG_REQUIRE(h && spfh_host, PRG_ERR_INVALID, "prg_fpfh_get_spfh: NULL argument");
    PRG_REQUIRE(h->have_spfh, PRG_ERR_STATE, "prg_fpfh_get_spfh: prg_fpfh_spfh first");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(spfh_host, h->spfh, h->n * kBins, h->stream));
    return PRG_OK;
}

int prg_fpfh_fpfh(prg_fpfh* h) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_fpfh_fpfh: NULL argument");
    PRG_REQUIRE(h->have_spfh && h->nb[1].valid, PRG_ERR_STATE, "prg_fpfh_fpfh: prg_fpfh_spfh first");
    PRG_ENTER(h->device);
    k_fpfh<<<(unsigned)h->n, kWave, 0, h->stream>>>(h->spfh.p, h->nb[1].idx.p, h->nb[1].d2.p, h->nb[1].cnt.p, h->nb[1].k, h->fpfh.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->have_fpfh = true;
    return PRG_OK;
}

int prg_fpfh_get_fpfh(prg_fpfh* h, double* fpfh_host) {
    PRG_REQUIRE(h && fpfh_host, PRG_ERR_INVALID, "prg_fpfh_get_fpfh: NULL argument");
    PRG_REQUIRE(h->have_fpfh, PRG_ERR_STATE, "prg_fpfh_get_fpfh: prg_fpfh_fpfh first");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(fpfh_host, h->fpfh, h->n * kBins, h->stream));
    return PRG_OK;
}

}  // extern "C"
