// Voxel down-sampling: Open3D's PointCloud::VoxelDownSample in fp64 with every sum in a stated order and no
// floating-point atomics.
//
//   k_minmax_*      per-axis minimum and maximum (exact in any order); the host derives lo = min - v / 2, checks the index range
//                   and counts the bits each axis needs
//   k_keys          cell indices floor((p - lo) / v), packed x | y | z into the bits in use (the packing keeps the lexicographic
//                   order of the definition's key c_x 2^42 + c_y 2^21 + c_z)
//   sort_pairs_u64  rocPRIM's stable radix sort over those bits only (lattice_sort.hip)
//   k_head_count, k_tile_scan, k_rows   run heads -> voxel row per sorted position, run starts, inverse, the voxel count V
//   k_block_pieces  piece sums of the runs that cross a boundary of the aligned blocks of kPiece sorted positions
//   k_voxel_means   per voxel: its one piece left to right, or its piece sums in ascending block order; mean = sum / count
//
// Every result is a function of the input alone: the pieces are cut at multiples of kPiece whatever the launch.
#include <algorithm>
#include <cmath>
#include <new>

#include "block_scan.h"
#include "dev_buf.h"
#include "lattice_sort.h"
#include "prg_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPiece = 64;                  // sorted positions per block of the two-level sums (part of the definition)
constexpr int kMaxChannels = 67;            // normals (3) and attributes (64) side by side
constexpr int kAxisBits = 21;
constexpr double kMaxCells = 2097152.0;     // 2^21 cells per axis
constexpr int kMinMaxBlocks = 1024;
constexpr int kScanPer = 4;                 // sorted positions per lane of the head scan
constexpr int kScanTile = kBlock * kScanPer;
constexpr int kScanThreads = 1024;

// ------------------------------------------------------------------------------------------------------------ min / max
// part: [block][6] = (min x, y, z, max x, y, z); the axes behind d report 0
__global__ __launch_bounds__(kBlock) void k_minmax_part(const double* __restrict__ pts, int64_t n, int d,
                                                        double* __restrict__ part) {
    __shared__ double s[6][kBlock];
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (a >= d) continue;
            const double x = pts[i * d + a];
            lo[a] = fmin(lo[a], x);
            hi[a] = fmax(hi[a], x);
        }
    for (int a = 0; a < 3; ++a) {
        s[a][threadIdx.x] = lo[a];
        s[3 + a][threadIdx.x] = hi[a];
    }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int a = 0; a < 3; ++a) {
                s[a][threadIdx.x] = fmin(s[a][threadIdx.x], s[a][threadIdx.x + w]);
                s[3 + a][threadIdx.x] = fmax(s[3 + a][threadIdx.x], s[3 + a][threadIdx.x + w]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) part[(int64_t)blockIdx.x * 6 + threadIdx.x] = s[threadIdx.x][0];
}

__global__ __launch_bounds__(kBlock) void k_minmax_final(const double* __restrict__ part, int nblocks, int d,
                                                         double* __restrict__ out) {
    __shared__ double s[6][kBlock];
    for (int a = 0; a < 6; ++a) {
        double v = a < 3 ? INFINITY : -INFINITY;
        for (int b = threadIdx.x; b < nblocks; b += kBlock) v = a < 3 ? fmin(v, part[b * 6 + a]) : fmax(v, part[b * 6 + a]);
        s[a][threadIdx.x] = v;
    }
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int a = 0; a < 6; ++a)
                s[a][threadIdx.x] = a < 3 ? fmin(s[a][threadIdx.x], s[a][threadIdx.x + w])
                                          : fmax(s[a][threadIdx.x], s[a][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x < 6) out[threadIdx.x] = (int)threadIdx.x % 3 < d ? s[threadIdx.x][0] : 0.0;
}

// ----------------------------------------------------------------------------------------------------------------- keys
// c = floor((p - lo) / v): a subtraction, a true division and a floor, each rounded once.  lo <= min, so c >= 0; the host has
// checked that the largest c of every axis is below 2^21.
__device__ __forceinline__ uint64_t cell_of(double p, double lo, double v) {
    return (uint64_t)floor(__ddiv_rn(__dsub_rn(p, lo), v));
}

struct KeyArgs {
    double lo[3];
    double v;
    int shift[3];  // bits to the right of the axis in the packed key
};

__global__ __launch_bounds__(kBlock) void k_keys(const double* __restrict__ pts, int64_t n, int d, KeyArgs ka,
                                                 uint64_t* __restrict__ keys, int* __restrict__ ident) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint64_t key = 0;
    for (int a = 0; a < d; ++a) key |= cell_of(pts[i * d + a], ka.lo[a], ka.v) << ka.shift[a];
    keys[i] = key;
    ident[i] = (int)i;
}

// ----------------------------------------------------------------------------------------------------- heads, rows, runs
// position j of the sorted sequence starts a run iff its key differs from the key before it
__device__ __forceinline__ bool is_head(const uint64_t* __restrict__ ks, int64_t j) { return j == 0 || ks[j] != ks[j - 1]; }

__device__ __forceinline__ int count_heads(const uint64_t* __restrict__ ks, int64_t n, int64_t b) {
    int c = 0;
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) c += (b + u < n && is_head(ks, b + u)) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(kBlock) void k_head_count(const uint64_t* __restrict__ ks, int64_t n, int* __restrict__ tile_count) {
    __shared__ int cnt[kBlock];
    cnt[threadIdx.x] = count_heads(ks, n, ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kScanPer);
    prg::scan_inclusive<kBlock>(cnt);
    if (threadIdx.x == kBlock - 1) tile_count[blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of the tile counts by one workgroup; *total = the number of voxels
__global__ __launch_bounds__(kScanThreads) void k_tile_scan(const int* __restrict__ tile_count, int ntiles,
                                                            int* __restrict__ tile_start, int* __restrict__ total) {
    __shared__ int cnt[kScanThreads];
    prg::tile_scan<kScanThreads>(tile_count, ntiles, tile_start, total, cnt);
}

// rows[j]: the voxel of sorted position j; start[r]: where run r begins, start[V] = n; inverse[order[j]] = rows[j]
__global__ __launch_bounds__(kBlock) void k_rows(const uint64_t* __restrict__ ks, const int* __restrict__ order, int64_t n,
                                                 const int* __restrict__ tile_start, int* __restrict__ rows,
                                                 int* __restrict__ start, int* __restrict__ inverse) {
    __shared__ int cnt[kBlock];
    const int64_t b = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kScanPer;
    const int c = count_heads(ks, n, b);
    cnt[threadIdx.x] = c;
    prg::scan_inclusive<kBlock>(cnt);
    int pos = tile_start[blockIdx.x] + cnt[threadIdx.x] - c;  // run heads before position b; position 0 is one, so a row is pos - 1 >= 0
#pragma unroll
    for (int u = 0; u < kScanPer; ++u) {
        const int64_t j = b + u;
        if (j >= n) break;
        if (is_head(ks, j)) start[pos++] = (int)j;
        rows[j] = pos - 1;
        inverse[order[j]] = pos - 1;
        if (j == n - 1) start[pos] = (int)n;
    }
}

// ----------------------------------------------------------------------------------------------------------------- sums
// src[order[j]][k] for j = j0 .. j1 - 1, left to right from 0.0; eight gathers in flight, the additions stay in order
__device__ __forceinline__ double piece_sum(const double* __restrict__ src, int K, int k, const int* __restrict__ order,
                                            int64_t j0, int64_t j1) {
    double acc = 0.0;
    int64_t j = j0;
    for (; j + 8 <= j1; j += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = src[(int64_t)order[j + u] * K + k];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __dadd_rn(acc, x[u]);
    }
    for (; j < j1; ++j) acc = __dadd_rn(acc, src[(int64_t)order[j] * K + k]);
    return acc;
}

// Lane (block b, column k).  Only runs that leave their block need stored pieces, and a block holds at most two of them: the
// piece at its first position (lead) and the piece at its last position (trail, when that is another run).  A run inside one
// block is summed by k_voxel_means directly.  lead / trail: [block][K]; an entry is written iff k_voxel_means reads it.
__global__ __launch_bounds__(kBlock) void k_block_pieces(const double* __restrict__ src, int K, const int* __restrict__ order,
                                                         const int* __restrict__ rows, const int* __restrict__ start,
                                                         int64_t n, int64_t nblocks, double* __restrict__ lead,
                                                         double* __restrict__ trail) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nblocks * K) return;
    const int64_t b = t / K;
    const int k = (int)(t - b * K);
    const int64_t p0 = b * kPiece;
    const int64_t p1 = p0 + kPiece < n ? p0 + kPiece : n;
    const int r_lead = rows[p0], r_trail = rows[p1 - 1];
    const int64_t lead_end = start[r_lead + 1];
    if (start[r_lead] < p0 || lead_end > p1) lead[t] = piece_sum(src, K, k, order, p0, lead_end < p1 ? lead_end : p1);
    if (r_trail != r_lead && start[r_trail + 1] > p1) trail[t] = piece_sum(src, K, k, order, start[r_trail], p1);
}

// Lane (voxel r, column k).  counts / first (may be null) are written by the lanes of column 0.
__global__ __launch_bounds__(kBlock) void k_voxel_means(const double* __restrict__ src, int K, const int* __restrict__ order,
                                                        const int* __restrict__ start, int64_t V,
                                                        const double* __restrict__ lead, const double* __restrict__ trail,
                                                        double* __restrict__ means, int* __restrict__ counts,
                                                        int* __restrict__ first) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= V * K) return;
    const int64_t r = t / K;
    const int k = (int)(t - r * K);
    const int64_t s = start[r], e = start[r + 1];
    const int64_t b0 = s / kPiece, b1 = (e - 1) / kPiece;
    double acc;
    if (b0 == b1) {
        acc = piece_sum(src, K, k, order, s, e);  // one piece: 0.0 + its sum is its sum
    } else {
        acc = __dadd_rn(0.0, (s % kPiece == 0 ? lead : trail)[b0 * K + k]);
        int64_t b = b0 + 1;
        for (; b + 8 <= b1; b += 8) {  // eight loads in flight; the additions stay in ascending block order
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = lead[(b + u) * K + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __dadd_rn(acc, x[u]);
        }
        for (; b <= b1; ++b) acc = __dadd_rn(acc, lead[b * K + k]);
    }
    means[t] = __ddiv_rn(acc, (double)(e - s));
    if (k == 0 && counts) counts[r] = (int)(e - s);
    if (k == 0 && first) first[r] = order[s];
}

int bits_of(uint64_t c) {
    int b = 0;
    while (c) {
        ++b;
        c >>= 1;
    }
    return b;
}

}  // namespace

struct prg_voxel {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0, V = 0;
    int d = 0, C = 0;
    bool have_result = false;
    int shift[3] = {0, 0, 0};             // of the last run's packed keys
    prg::DevBuf<double> pts, chan;        // [n][d], [n][C]
    prg::DevBuf<double> mm_part, mm;      // [kMinMaxBlocks][6], [6]
    prg::DevBuf<uint64_t> keys, keys_sorted;
    prg::DevBuf<int> ident, order, rows, start, inverse;
    prg::DevBuf<int> tile_count, tile_start, v_dev;
    prg::DevBuf<char> sort_tmp;
    prg::DevBuf<double> lead, trail;      // [blocks][max(d, C)]
    prg::DevBuf<double> means, chan_means;
    prg::DevBuf<int> counts, first;
};

namespace {

int sums_of(prg_voxel* h, const double* src, int K, double* means, bool with_counts) {
    const int64_t nblocks = prg::ceil_div(h->n, kPiece);
    k_block_pieces<<<(unsigned)prg::ceil_div(nblocks * K, kBlock), kBlock, 0, h->stream>>>(
        src, K, h->order.p, h->rows.p, h->start.p, h->n, nblocks, h->lead.p, h->trail.p);
    k_voxel_means<<<(unsigned)prg::ceil_div(h->V * K, kBlock), kBlock, 0, h->stream>>>(
        src, K, h->order.p, h->start.p, h->V, h->lead.p, h->trail.p, means, with_counts ? h->counts.p : nullptr,
        with_counts ? h->first.p : nullptr);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

template <class T>
int fetch(prg_voxel* h, const char* who, T* host, const prg::DevBuf<T>* dev, int64_t count) {
    PRG_REQUIRE(h && host, PRG_ERR_INVALID, "%s: NULL argument", who);
    PRG_REQUIRE(h->have_result, PRG_ERR_STATE, "%s: prg_voxel_run first", who);
    PRG_ENTER_AS(who, h->device);
    return prg::copy_out(host, *dev, count, h->stream);
}

}  // namespace

extern "C" {

int prg_voxel_create(prg_voxel** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_voxel_destroy(prg_voxel* h) {
    return prg::destroy_handle(h);
}

int prg_voxel_set_data(prg_voxel* h, const double* points_hd, int64_t n, int d) {
    PRG_REQUIRE(d == 2 || d == 3, PRG_ERR_INVALID, "prg_voxel_set_data: d must be 2 or 3, got %d", d);
    PRG_REQUIRE(n >= 1 && n < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_voxel_set_data: need 1 <= n < 2^31 points, got %lld",
                (long long)n);
    PRG_REQUIRE(h && points_hd, PRG_ERR_INVALID, "prg_voxel_set_data: NULL argument");
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->n = 0;
    h->C = 0;
    h->have_result = false;
    PRG_HIP(h->pts.ensure(n * d, n * d));
    PRG_HIP(hipMemcpyAsync(h->pts.p, points_hd, (size_t)n * d * sizeof(double), hipMemcpyDefault, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->n = n;
    h->d = d;
    return PRG_OK;
}

int prg_voxel_set_channels(prg_voxel* h, const double* channels_hd, int c) {
    PRG_REQUIRE(c >= 0 && c <= kMaxChannels, PRG_ERR_INVALID, "prg_voxel_set_channels: c must lie in 0 .. %d, got %d",
                kMaxChannels, c);
    PRG_REQUIRE(h && (c == 0 || channels_hd), PRG_ERR_INVALID, "prg_voxel_set_channels: NULL argument");
    PRG_REQUIRE(h->n >= 1, PRG_ERR_STATE, "prg_voxel_set_channels: no points (prg_voxel_set_data first)");
    PRG_ENTER(h->device);
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->C = 0;
    h->have_result = false;
    if (c == 0) return PRG_OK;
    PRG_HIP(h->chan.ensure(h->n * c, h->n * c));
    PRG_HIP(hipMemcpyAsync(h->chan.p, channels_hd, (size_t)h->n * c * sizeof(double), hipMemcpyDefault, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    h->C = c;
    return PRG_OK;
}

int prg_voxel_run(prg_voxel* h, double v) {
    PRG_REQUIRE(std::isfinite(v) && v > 0.0, PRG_ERR_INVALID, "prg_voxel_run: voxel_size must be finite and > 0, got %g", v);
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_voxel_run: NULL argument");
    PRG_REQUIRE(h->n >= 1, PRG_ERR_STATE, "prg_voxel_run: no points (prg_voxel_set_data first)");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    const int64_t n = h->n;
    const int d = h->d;
    PRG_HIP(hipStreamSynchronize(st));
    h->have_result = false;
    h->V = 0;

    // 1. the box; the index range is checked before anything is sorted
    const int mm_blocks = (int)std::min<int64_t>(prg::ceil_div(n, kBlock), kMinMaxBlocks);
    PRG_HIP(h->mm_part.ensure((int64_t)kMinMaxBlocks * 6, (int64_t)kMinMaxBlocks * 6));
    PRG_HIP(h->mm.ensure(6, 6));
    k_minmax_part<<<mm_blocks, kBlock, 0, st>>>(h->pts.p, n, d, h->mm_part.p);
    k_minmax_final<<<1, kBlock, 0, st>>>(h->mm_part.p, mm_blocks, d, h->mm.p);
    PRG_HIP(hipGetLastError());
    double mm[6];
    PRG_HIP(hipMemcpyAsync(mm, h->mm.p, sizeof(mm), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    KeyArgs ka;
    ka.v = v;
    int bits[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        ka.lo[a] = 0.0;
        if (a >= d) continue;
        const double half = 0.5 * v;
        ka.lo[a] = mm[a] - half;
        const double cmax = std::floor((mm[3 + a] - ka.lo[a]) / v);  // the cell index is monotone in p
        PRG_REQUIRE(cmax < kMaxCells, PRG_ERR_INVALID,
                    "prg_voxel_run: axis %d (%c) has extent %g, which voxel_size %g cuts into %.17g cells; the limit is 2^%d = "
                    "%.0f cells per axis",
                    a, "xyz"[a], mm[3 + a] - mm[a], v, cmax + 1.0, kAxisBits, kMaxCells);
        bits[a] = bits_of((uint64_t)cmax);
    }
    ka.shift[2] = 0;
    ka.shift[1] = bits[2];
    ka.shift[0] = bits[2] + bits[1];
    const unsigned key_bits = (unsigned)std::max(1, bits[0] + bits[1] + bits[2]);

    // 2. keys, 3. sort
    const int ntiles = (int)prg::ceil_div(n, kScanTile);
    PRG_HIP(h->keys.ensure(n, n));
    PRG_HIP(h->keys_sorted.ensure(n, n));
    PRG_HIP(h->ident.ensure(n, n));
    PRG_HIP(h->order.ensure(n, n));
    PRG_HIP(h->rows.ensure(n, n));
    PRG_HIP(h->start.ensure(n + 1, n + 1));
    PRG_HIP(h->inverse.ensure(n, n));
    PRG_HIP(h->tile_count.ensure(ntiles, ntiles));
    PRG_HIP(h->tile_start.ensure(ntiles, ntiles));
    PRG_HIP(h->v_dev.ensure(1, 1));
    size_t tmp_bytes = 0;
    PRG_TRY(prg::sort_pairs_u64(nullptr, &tmp_bytes, h->keys.p, h->keys_sorted.p, h->ident.p, h->order.p, (unsigned)n, key_bits,
                                st));
    PRG_HIP(h->sort_tmp.ensure((int64_t)std::max<size_t>(tmp_bytes, 1), (int64_t)std::max<size_t>(tmp_bytes, 1)));
    for (int a = 0; a < 3; ++a) h->shift[a] = ka.shift[a];
    k_keys<<<(unsigned)prg::ceil_div(n, kBlock), kBlock, 0, st>>>(h->pts.p, n, d, ka, h->keys.p, h->ident.p);
    PRG_HIP(hipGetLastError());
    PRG_TRY(prg::sort_pairs_u64(h->sort_tmp.p, &tmp_bytes, h->keys.p, h->keys_sorted.p, h->ident.p, h->order.p, (unsigned)n,
                                key_bits, st));

    // 4. run heads -> rows, run starts, inverse, V
    k_head_count<<<ntiles, kBlock, 0, st>>>(h->keys_sorted.p, n, h->tile_count.p);
    k_tile_scan<<<1, kScanThreads, 0, st>>>(h->tile_count.p, ntiles, h->tile_start.p, h->v_dev.p);
    k_rows<<<ntiles, kBlock, 0, st>>>(h->keys_sorted.p, h->order.p, n, h->tile_start.p, h->rows.p, h->start.p, h->inverse.p);
    PRG_HIP(hipGetLastError());
    int V = 0;
    PRG_HIP(hipMemcpyAsync(&V, h->v_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    PRG_REQUIRE(V >= 1 && V <= n, PRG_ERR_STATE, "prg_voxel_run: internal error, %d voxels of %lld points", V, (long long)n);
    h->V = V;

    // 5. / 6. sums and means, channel by channel in the same order
    const int64_t nblocks = prg::ceil_div(n, kPiece);
    const int kmax = std::max(d, h->C);
    PRG_HIP(h->lead.ensure(nblocks * kmax, nblocks * kmax));
    PRG_HIP(h->trail.ensure(nblocks * kmax, nblocks * kmax));
    PRG_HIP(h->means.ensure((int64_t)V * d, (int64_t)V * d));
    PRG_HIP(h->counts.ensure(V, V));
    PRG_HIP(h->first.ensure(V, V));
    PRG_TRY(sums_of(h, h->pts.p, d, h->means.p, true));
    if (h->C > 0) {
        PRG_HIP(h->chan_means.ensure((int64_t)V * h->C, (int64_t)V * h->C));
        PRG_TRY(sums_of(h, h->chan.p, h->C, h->chan_means.p, false));
    }
    h->have_result = true;
    return PRG_OK;
}

int prg_voxel_count(prg_voxel* h, int64_t* v_host) {
    PRG_REQUIRE(h && v_host, PRG_ERR_INVALID, "prg_voxel_count: NULL argument");
    PRG_REQUIRE(h->have_result, PRG_ERR_STATE, "prg_voxel_count: prg_voxel_run first");
    *v_host = h->V;
    return PRG_OK;
}

int prg_voxel_get_means(prg_voxel* h, double* means_host) {
    return fetch(h, "prg_voxel_get_means", means_host, h ? &h->means : nullptr, h ? h->V * h->d : 0);
}

int prg_voxel_get_channel_means(prg_voxel* h, double* means_host) {
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_voxel_get_channel_means: NULL argument");
    PRG_REQUIRE(!h->have_result || h->C > 0, PRG_ERR_STATE, "prg_voxel_get_channel_means: no channels (prg_voxel_set_channels)");
    return fetch(h, "prg_voxel_get_channel_means", means_host, &h->chan_means, h->V * h->C);
}

int prg_voxel_get_counts(prg_voxel* h, int* counts_host) {
    return fetch(h, "prg_voxel_get_counts", counts_host, h ? &h->counts : nullptr, h ? h->V : 0);
}

int prg_voxel_get_first(prg_voxel* h, int* first_host) {
    return fetch(h, "prg_voxel_get_first", first_host, h ? &h->first : nullptr, h ? h->V : 0);
}

int prg_voxel_get_inverse(prg_voxel* h, int* inverse_host) {
    return fetch(h, "prg_voxel_get_inverse", inverse_host, h ? &h->inverse : nullptr, h ? h->n : 0);
}

int prg_voxel_get_keys(prg_voxel* h, uint64_t* keys_host) {
    PRG_TRY(fetch(h, "prg_voxel_get_keys", keys_host, h ? &h->keys : nullptr, h ? h->n : 0));
    // packed x | y | z in the bits in use -> the definition's c_x 2^42 + c_y 2^21 + c_z
    const int sx = h->shift[0], sy = h->shift[1];
    for (int64_t i = 0; i < h->n; ++i) {
        const uint64_t p = keys_host[i];
        const uint64_t cx = p >> sx, cy = (p >> sy) & ((1ull << (sx - sy)) - 1), cz = p & ((1ull << sy) - 1);
        keys_host[i] = (cx << (2 * kAxisBits)) | (cy << kAxisBits) | cz;
    }
    return PRG_OK;
}

int prg_voxel_get_order(prg_voxel* h, int* order_host) {
    return fetch(h, "prg_voxel_get_order", order_host, h ? &h->order : nullptr, h ? h->n : 0);
}

int prg_voxel_get_rows(prg_voxel* h, int* rows_host) {
    return fetch(h, "prg_voxel_get_rows", rows_host, h ? &h->rows : nullptr, h ? h->n : 0);
}

}  // extern "C"
