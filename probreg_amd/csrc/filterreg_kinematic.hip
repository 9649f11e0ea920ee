// Deformable kinematic FilterReg (reference probreg/filterreg.py:199-266, transformation.py:163-212) for gfx950:
// dual-quaternion linear blending of two nodes per point, and the per-node-pair sums of the Gauss-Newton M-step
// (DESIGN.md section 3.10).  Everything is fp64; every sum has a fixed order (chunk partials, then the chunks of a
// segment in order), no atomics on floating-point data.
//
// The points are sorted ONCE by ordered pair key (pair0 * K + pair1, stable) when the skinning weights are set; a
// "segment" is the run of one key, cut into chunks of kChunk points.  One workgroup reduces one chunk, one more
// launch adds the chunks of every segment.  The 6K x 6K assembly and the minimum-norm solve stay on the host.
#include <float.h>
#include <math.h>

#include <algorithm>
#include <new>
#include <vector>

#include "dev_buf.h"
#include "fr_plan.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 512;
constexpr int kNrm = 34;  // 0..9 w0^2 * s^2 * (1,x,y,z,xx,xy,xz,yy,yz,zz) | 10..19 w0 w1 | 20..29 w1^2 | 30 sigma2 numerator | 31 sum m0/(m0+c) | 32 live points | 33 -
constexpr int kGrd = 16;  // 0..5 w0 * s * J^T rx | 6..11 w1 * s * J^T rx | 12 q | 13..15 -

struct Chunk { int first, last, seg, pad; };  // sorted positions [first, last) of segment seg

// ---- dual quaternions (r_w, r_x, r_y, r_z, d_w, d_x, d_y, d_z) --------------------------------------------------------
// dualquat_from_twist (filterreg.py:38-42): rotation by |tw[:3]| about tw[:3], translation tw[3:]; d = (0, t) r / 2
__device__ __forceinline__ void dq_from_twist(const double* tw, double* q) {
    const double ang = sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
    double r[4] = {1.0, 0.0, 0.0, 0.0};
    if (!(ang < (double)FLT_EPSILON)) {
        const double s = sin(0.5 * ang) / ang;
        r[0] = cos(0.5 * ang);
        r[1] = s * tw[0]; r[2] = s * tw[1]; r[3] = s * tw[2];
    }
    const double* t = tw + 3;
    q[0] = r[0]; q[1] = r[1]; q[2] = r[2]; q[3] = r[3];
    q[4] = 0.5 * (-(t[0] * r[1] + t[1] * r[2] + t[2] * r[3]));
    q[5] = 0.5 * (t[0] * r[0] + t[1] * r[3] - t[2] * r[2]);
    q[6] = 0.5 * (t[1] * r[0] + t[2] * r[1] - t[0] * r[3]);
    q[7] = 0.5 * (t[2] * r[0] + t[0] * r[2] - t[1] * r[1]);
}

// DLB of two nodes, both parts divided by |b.r| (no antipodal sign correction), then
// p -> vec(r (0,p) r*) + 2 vec(d r*)
__device__ __forceinline__ void skin_point(const double* __restrict__ dq, int p0, int p1, double w0, double w1,
                                           const double* p, double* x) {
    double b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] = w0 * dq[8 * p0 + k] + w1 * dq[8 * p1 + k];
    const double inv = 1.0 / sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
#pragma unroll
    for (int k = 0; k < 8; ++k) b[k] *= inv;
    const double rw = b[0], vx = b[1], vy = b[2], vz = b[3];
    // rotation: p + 2 w (v x p) + 2 v x (v x p)
    const double cx = vy * p[2] - vz * p[1], cy = vz * p[0] - vx * p[2], cz = vx * p[1] - vy * p[0];
    const double ex = vy * cz - vz * cy, ey = vz * cx - vx * cz, ez = vx * cy - vy * cx;
    // translation: 2 vec(d r*) = 2 (r_w d_v - d_w r_v - d_v x r_v)
    const double dw = b[4], dx = b[5], dy = b[6], dz = b[7];
    const double tx = rw * dx - dw * vx - (dy * vz - dz * vy);
    const double ty = rw * dy - dw * vy - (dz * vx - dx * vz);
    const double tz = rw * dz - dw * vz - (dx * vy - dy * vx);
    x[0] = p[0] + 2.0 * (rw * cx + ex) + 2.0 * tx;
    x[1] = p[1] + 2.0 * (rw * cy + ey) + 2.0 * ty;
    x[2] = p[2] + 2.0 * (rw * cz + ez) + 2.0 * tz;
}

__global__ void k_dq_from_twist(const double* __restrict__ tw, int k_nodes, double* __restrict__ dq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k_nodes) dq_from_twist(tw + 6 * i, dq + 8 * i);
}

// stateless skinning in the caller's order (transformation.py:209-212)
__global__ __launch_bounds__(kBlock) void k_dq_skin(const double* __restrict__ pts, const int* __restrict__ pairs,
                                                    const float* __restrict__ wts, const double* __restrict__ dq,
                                                    int64_t m, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const double p[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
    double x[3];
    skin_point(dq, pairs[2 * i], pairs[2 * i + 1], (double)wts[2 * i], (double)wts[2 * i + 1], p, x);
    out[3 * i] = x[0]; out[3 * i + 1] = x[1]; out[3 * i + 2] = x[2];
}

// the plan's source (4 doubles per point, plan order) -> moved source, same layout; j runs over the key-sorted order
__global__ __launch_bounds__(kBlock) void k_kin_skin(const double* __restrict__ src, const int* __restrict__ ord,
                                                     const int2* __restrict__ kp, const double2* __restrict__ kw,
                                                     const double* __restrict__ dq, int64_t m, double* __restrict__ moved) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const int64_t i = ord[j];
    const double p[3] = {src[4 * i], src[4 * i + 1], src[4 * i + 2]};
    double x[3];
    skin_point(dq, kp[j].x, kp[j].y, kw[j].x, kw[j].y, p, x);
    moved[4 * i] = x[0]; moved[4 * i + 1] = x[1]; moved[4 * i + 2] = x[2]; moved[4 * i + 3] = 0.0;
}

// ---- fixed-order workgroup sum ----------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
template <int NC>
__device__ __forceinline__ void block_sum_store(const double* acc, double* __restrict__ out) {
    __shared__ double sh[kBlock / 64][NC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double v = wave_sum(acc[c]);
        if (lane == 0) sh[wave][c] = v;
    }
    __syncthreads();
    if (threadIdx.x < NC) out[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// where the E-step's values of a point lie: the plan's interleaved `vout` or the caller's separate arrays
struct EstepIn {
    const double* ts; int ts_stride;
    const float* m0; int m0_stride;
    const float* m1; int m1_stride;
    const float* m2; int m2_stride;  // null: sigma2 is not re-estimated
};

// Normal-matrix sums, once per M-step (filterreg.py:222-236): per point s = sqrt(m0/(m0+c)/sigma2), mu = m1/m0, and
// s^2 * (1, x, xx^T) of the moved source x under w0^2, w0 w1, w1^2 - the 21 entries of J^T J, J = [-[x]x | I], are
// linear in those ten moments.  Also keeps (x, s) and mu per point, in sorted order, for the gradient sums.
__global__ __launch_bounds__(kBlock) void k_kin_normal(const Chunk* __restrict__ chunks, const int* __restrict__ ord,
                                                       const EstepIn in, const double2* __restrict__ kw, double c,
                                                       double sigma2, int reference_form, double4* __restrict__ pt,
                                                       double4* __restrict__ mu, double* __restrict__ part) {
    const Chunk ck = chunks[blockIdx.x];
    double acc[kNrm];
#pragma unroll
    for (int k = 0; k < kNrm; ++k) acc[k] = 0.0;
    for (int j = ck.first + (int)threadIdx.x; j < ck.last; j += kBlock) {
        const int64_t i = ord[j];
        const double x[3] = {in.ts[i * in.ts_stride], in.ts[i * in.ts_stride + 1], in.ts[i * in.ts_stride + 2]};
        double m0 = (double)in.m0[i * in.m0_stride];
        const double m1[3] = {(double)in.m1[i * in.m1_stride], (double)in.m1[i * in.m1_stride + 1],
                              (double)in.m1[i * in.m1_stride + 2]};
        bool live = true;
        if (m0 == 0.0) {
            if (reference_form) m0 = (double)FLT_EPSILON;  // filterreg.py:223
            else live = false;
        }
        double s = 0.0, mx = 0.0, my = 0.0, mz = 0.0;
        if (live) {
            const double m0m0 = m0 / (m0 + c);
            s = sqrt(m0m0 * 1.0 / sigma2);
            mx = m1[0] / m0; my = m1[1] / m0; mz = m1[2] / m0;
            const double m2 = in.m2 ? (double)in.m2[i * in.m2_stride] : 0.0;
            acc[30] += (m0 * (x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) - 2.0 * (x[0] * m1[0] + x[1] * m1[1] + x[2] * m1[2]) + m2) / (m0 + c);
            acc[31] += m0m0;
            acc[32] += 1.0;
        }
        pt[j] = make_double4(x[0], x[1], x[2], s);
        mu[j] = make_double4(mx, my, mz, 0.0);
        const double s2 = s * s;
        const double mom[10] = {s2, s2 * x[0], s2 * x[1], s2 * x[2], s2 * x[0] * x[0], s2 * x[0] * x[1], s2 * x[0] * x[2],
                                s2 * x[1] * x[1], s2 * x[1] * x[2], s2 * x[2] * x[2]};
        const double2 w = kw[j];
        // (reference form: `w[0] * w[1]` of two f4 values is an f4 product in the reference, filterreg.py:233-234)
        const double ww[3] = {w.x * w.x, reference_form ? (double)((float)w.x * (float)w.y) : w.x * w.y, w.y * w.y};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 10; ++k) acc[10 * a + k] += ww[a] * mom[k];
    }
    block_sum_store<kNrm>(acc, part + (int64_t)blockIdx.x * kNrm);
}

// Gradient sums, once per inner iteration (filterreg.py:238-254, 265): skin with the current increments, rx = s (x - mu),
// s J^T rx = s (t x rx ; rx) with J evaluated at the moved source t, under w0 and w1; q = sum_i (rx_0 + rx_1 + rx_2)^2
__global__ __launch_bounds__(kBlock) void k_kin_grad(const Chunk* __restrict__ chunks, const double4* __restrict__ pt,
                                                     const double4* __restrict__ mu, const int2* __restrict__ kp,
                                                     const double2* __restrict__ kw, const double* __restrict__ dq,
                                                     int reference_form, double* __restrict__ part) {
    const Chunk ck = chunks[blockIdx.x];
    double acc[kGrd];
#pragma unroll
    for (int k = 0; k < kGrd; ++k) acc[k] = 0.0;
    for (int j = ck.first + (int)threadIdx.x; j < ck.last; j += kBlock) {
        const double4 t4 = pt[j], m4 = mu[j];
        const int2 p = kp[j];
        const double2 w = kw[j];
        const double t[3] = {t4.x, t4.y, t4.z};
        double x[3] = {0.0, 0.0, 0.0};
        // (the reference walks itertools.permutations: a point whose two nodes coincide is never skinned, :238-244)
        if (!(reference_form && p.x == p.y)) skin_point(dq, p.x, p.y, w.x, w.y, t, x);
        const double s = t4.w;
        const double rx[3] = {s * (x[0] - m4.x), s * (x[1] - m4.y), s * (x[2] - m4.z)};
        const double g[6] = {s * (t[1] * rx[2] - t[2] * rx[1]), s * (t[2] * rx[0] - t[0] * rx[2]),
                             s * (t[0] * rx[1] - t[1] * rx[0]), s * rx[0], s * rx[1], s * rx[2]};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            acc[k] += w.x * g[k];
            acc[6 + k] += w.y * g[k];
        }
        const double r = rx[0] + rx[1] + rx[2];
        acc[12] += r * r;
    }
    block_sum_store<kGrd>(acc, part + (int64_t)blockIdx.x * kGrd);
}

// the chunks of every segment, added in order
__global__ void k_kin_segsum(const double* __restrict__ part, const int* __restrict__ seg_chunk, int nc,
                             double* __restrict__ out) {
    const int s = blockIdx.x, c = threadIdx.x;
    if (c >= nc) return;
    double v = 0.0;
    for (int k = seg_chunk[s]; k < seg_chunk[s + 1]; ++k) v += part[(int64_t)k * nc + c];
    out[(int64_t)s * nc + c] = v;
}

struct Kin {
    int64_t M = 0;
    int K = 0, S = 0, n_chunks = 0;
    // one group (dev_buf.h: reset_group), created by build_kin for the life of the Kin
    prg::DevBuf<int> ord_plan;    // [M] sorted position -> plan position
    prg::DevBuf<int> ord_caller;  // [M] sorted position -> caller's index
    prg::DevBuf<int2> kp;         // [M] node pair, sorted order
    prg::DevBuf<double2> kw;      // [M] weights widened to fp64, sorted order
    prg::DevBuf<Chunk> chunks;    // [n_chunks]
    prg::DevBuf<int> seg_chunk;   // [S + 1]
    prg::DevBuf<double4> pt;      // [M] (moved source, s), sorted order
    prg::DevBuf<double4> mu;      // [M] m1 / m0, sorted order
    prg::DevBuf<double> part;     // [n_chunks][kNrm]
    prg::DevBuf<double> segsum;   // [S][kNrm]
    prg::DevBuf<double> dq;       // [K][8] the model's dual quaternions
    prg::DevBuf<double> dq_inc;   // [K][8] dualquat_from_twist of the inner loop's increments
    prg::DevBuf<double> tw;       // [6 K]
    prg::DevBuf<double> moved;    // [M][4] skinned source, plan order
    std::vector<double> dq_host;
    // E-step values supplied by the caller (prg_fr_kinematic_set_arrays) instead of the plan's last E-step
    prg::DevBuf<char> arrays;  // allocated once
    EstepIn arr_in{};
    int64_t arr_n_target = 0;
    bool use_arrays = false, have_normal = false;
};

void kin_free(void* p) { delete (Kin*)p; }

// an uploaded array has at least one element
template <typename T>
int64_t slots(const std::vector<T>& host) {
    return (int64_t)std::max<size_t>(host.size(), 1);
}

template <typename T>
int upload(const prg::DevBuf<T>& dev, const std::vector<T>& host, hipStream_t st) {
    if (!host.empty()) PRG_HIP(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return PRG_OK;
}

int check_pairs(const char* who, const std::vector<int>& pairs, int k_nodes) {
    for (size_t i = 0; i < pairs.size(); ++i)
        PRG_REQUIRE(pairs[i] >= 0 && pairs[i] < k_nodes, PRG_ERR_INVALID, "%s: node index %d of point %lld is outside [0, %d)",
                    who, pairs[i], (long long)(i / 2), k_nodes);
    return PRG_OK;
}

int build_kin(Kin* k, const prg::FrView& v, const std::vector<int>& pairs, const std::vector<float>& wts, int k_nodes) {
    const int64_t m = v.M;
    hipStream_t st = v.stream;
    k->M = m;
    k->K = k_nodes;
    std::vector<int> order((size_t)m);
    std::vector<long long> key((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        order[(size_t)i] = (int)i;
        key[(size_t)i] = (long long)pairs[2 * i] * k_nodes + pairs[2 * i + 1];
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[(size_t)a] < key[(size_t)b]; });
    std::vector<int> pos_of;  // caller's index -> plan position
    if (v.src_order) {
        pos_of.resize((size_t)m);
        for (int64_t i = 0; i < m; ++i) pos_of[(size_t)v.src_order[i]] = (int)i;
    }
    std::vector<int> ord_plan((size_t)m), seg_chunk;
    std::vector<int2> kp((size_t)m);
    std::vector<double2> kw((size_t)m);
    std::vector<Chunk> chunks;
    int n_seg = 0;
    for (int64_t j = 0; j < m;) {
        int64_t e = j;
        while (e < m && key[(size_t)order[(size_t)e]] == key[(size_t)order[(size_t)j]]) ++e;
        seg_chunk.push_back((int)chunks.size());
        for (int64_t a = j; a < e; a += kChunk) chunks.push_back(Chunk{(int)a, (int)std::min<int64_t>(a + kChunk, e), n_seg, 0});
        ++n_seg;
        j = e;
    }
    seg_chunk.push_back((int)chunks.size());
    for (int64_t j = 0; j < m; ++j) {
        const int i = order[(size_t)j];
        ord_plan[(size_t)j] = pos_of.empty() ? i : pos_of[(size_t)i];
        kp[(size_t)j] = make_int2(pairs[2 * (size_t)i], pairs[2 * (size_t)i + 1]);
        kw[(size_t)j] = make_double2((double)wts[2 * (size_t)i], (double)wts[2 * (size_t)i + 1]);  // f4 in the reference: widened here
    }
    k->S = n_seg;
    k->n_chunks = (int)chunks.size();
    k->dq_host.assign((size_t)k_nodes * 8, 0.0);
    for (int i = 0; i < k_nodes; ++i) k->dq_host[(size_t)i * 8] = 1.0;
    PRG_HIP(prg::reset_group(k->ord_plan, slots(ord_plan), k->ord_caller, slots(order), k->kp, slots(kp), k->kw, slots(kw), k->chunks,
                             slots(chunks), k->seg_chunk, slots(seg_chunk), k->pt, m, k->mu, m, k->part, (int64_t)k->n_chunks * kNrm,
                             k->segsum, (int64_t)k->S * kNrm, k->dq_inc, (int64_t)k_nodes * 8, k->tw, (int64_t)k_nodes * 6, k->moved,
                             m * 4, k->dq, slots(k->dq_host)));
    PRG_TRY(upload(k->ord_plan, ord_plan, st));
    PRG_TRY(upload(k->ord_caller, order, st));
    PRG_TRY(upload(k->kp, kp, st));
    PRG_TRY(upload(k->kw, kw, st));
    PRG_TRY(upload(k->chunks, chunks, st));
    PRG_TRY(upload(k->seg_chunk, seg_chunk, st));
    PRG_TRY(upload(k->dq, k->dq_host, st));
    PRG_HIP(hipStreamSynchronize(st));  // the host vectors go out of scope
    return PRG_OK;
}

Kin* kin_of(const prg::FrView& v) { return (Kin*)*v.kin; }

// segment sums [S][nc] of chunk partials -> host
int seg_sums_to_host(Kin* k, int nc, hipStream_t st, double* out_host) {
    k_kin_segsum<<<k->S, 64, 0, st>>>(k->part.p, k->seg_chunk.p, nc, k->segsum.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(out_host, k->segsum.p, (size_t)k->S * nc * sizeof(double), hipMemcpyDeviceToHost, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

}  // namespace

extern "C" {

int prg_dq_skin(int device, void* hip_stream, const double* points_hd, int64_t m, const int* pairs_hd,
                const float* weights_hd, const double* dualquats_hd, int k_nodes, double* out_hd) {
    PRG_REQUIRE(points_hd && pairs_hd && weights_hd && dualquats_hd && out_hd, PRG_ERR_INVALID, "prg_dq_skin: NULL argument");
    PRG_REQUIRE(m > 0 && m < (1ll << 31) && k_nodes > 0, PRG_ERR_INVALID, "prg_dq_skin: need 0 < m < 2^31 and k_nodes > 0");
    PRG_ENTER(device);
    hipStream_t st = (hipStream_t)hip_stream;
    std::vector<int> pairs((size_t)m * 2);
    PRG_HIP(hipMemcpy(pairs.data(), pairs_hd, pairs.size() * sizeof(int), hipMemcpyDefault));
    PRG_TRY(check_pairs("prg_dq_skin", pairs, k_nodes));
    prg::DevBuf<double> b_pts, b_dq, b_out;
    prg::DevBuf<int> b_pairs;
    prg::DevBuf<float> b_w;
    PRG_HIP(b_pts.reset(m * 3));
    PRG_HIP(b_pairs.reset(m * 2));
    PRG_HIP(b_w.reset(m * 2));
    PRG_HIP(b_dq.reset((int64_t)k_nodes * 8));
    PRG_HIP(b_out.reset(m * 3));
    PRG_HIP(hipMemcpyAsync(b_pts.p, points_hd, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(b_pairs.p, pairs.data(), (size_t)m * 2 * sizeof(int), hipMemcpyHostToDevice, st));
    PRG_HIP(hipMemcpyAsync(b_w.p, weights_hd, (size_t)m * 2 * sizeof(float), hipMemcpyDefault, st));
    PRG_HIP(hipMemcpyAsync(b_dq.p, dualquats_hd, (size_t)k_nodes * 8 * sizeof(double), hipMemcpyDefault, st));
    k_dq_skin<<<(unsigned)prg::ceil_div(m, kBlock), kBlock, 0, st>>>(b_pts.p, b_pairs.p, b_w.p, b_dq.p, m, b_out.p);
    PRG_HIP(hipGetLastError());
    PRG_HIP(hipMemcpyAsync(out_hd, b_out.p, (size_t)m * 3 * sizeof(double), hipMemcpyDefault, st));
    PRG_HIP(hipStreamSynchronize(st));
    return PRG_OK;
}

int prg_fr_set_skinning(prg_filterreg* h, const int* pairs_hd, const float* weights_hd, int64_t m, int k_nodes,
                        int* n_segments) {
    PRG_REQUIRE(h && pairs_hd && weights_hd, PRG_ERR_INVALID, "prg_fr_set_skinning: NULL argument");
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, false));
    PRG_REQUIRE(v.have_src, PRG_ERR_STATE, "prg_fr_set_skinning: set the source first");
    PRG_REQUIRE(v.D == 3, PRG_ERR_INVALID, "prg_fr_set_skinning: the kinematic model needs 3-D clouds");
    PRG_REQUIRE(m == v.M, PRG_ERR_INVALID, "prg_fr_set_skinning: %lld weights for %lld source points", (long long)m, (long long)v.M);
    PRG_REQUIRE(k_nodes > 0 && k_nodes <= 32768, PRG_ERR_INVALID, "prg_fr_set_skinning: need 0 < k_nodes <= 32768");
    PRG_ENTER(v.device);
    std::vector<int> pairs((size_t)m * 2);
    std::vector<float> wts((size_t)m * 2);
    PRG_HIP(hipMemcpy(pairs.data(), pairs_hd, pairs.size() * sizeof(int), hipMemcpyDefault));
    PRG_HIP(hipMemcpy(wts.data(), weights_hd, wts.size() * sizeof(float), hipMemcpyDefault));
    PRG_TRY(check_pairs("prg_fr_set_skinning", pairs, k_nodes));  // (an earlier skinning stays in place on failure)
    PRG_HIP(hipStreamSynchronize(v.stream));
    Kin* k = new (std::nothrow) Kin();
    PRG_REQUIRE(k != nullptr, PRG_ERR_NOMEM, "prg_fr_set_skinning: out of host memory");
    const int st = build_kin(k, v, pairs, wts, k_nodes);
    if (st != PRG_OK) {
        kin_free(k);
        return st;
    }
    if (*v.kin) kin_free(*v.kin);
    *v.kin = k;
    *v.kin_free = kin_free;
    if (n_segments) *n_segments = k->S;
    return PRG_OK;
}

int prg_fr_set_dualquats(prg_filterreg* h, const double* dualquats_host, int k_nodes) {
    PRG_REQUIRE(h && dualquats_host, PRG_ERR_INVALID, "prg_fr_set_dualquats: NULL argument");
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, false));
    Kin* k = kin_of(v);
    PRG_REQUIRE(k, PRG_ERR_STATE, "prg_fr_set_dualquats: set the skinning weights first");
    PRG_REQUIRE(k_nodes == k->K, PRG_ERR_INVALID, "prg_fr_set_dualquats: %d dual quaternions for %d nodes", k_nodes, k->K);
    PRG_ENTER(v.device);
    k->dq_host.assign(dualquats_host, dualquats_host + (size_t)k_nodes * 8);
    PRG_HIP(hipMemcpyAsync(k->dq.p, k->dq_host.data(), k->dq_host.size() * sizeof(double), hipMemcpyHostToDevice, v.stream));
    PRG_HIP(hipStreamSynchronize(v.stream));
    return PRG_OK;
}

int prg_fr_get_dualquats(prg_filterreg* h, double* dualquats_host, int k_nodes) {
    PRG_REQUIRE(h && dualquats_host, PRG_ERR_INVALID, "prg_fr_get_dualquats: NULL argument");
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, false));
    Kin* k = kin_of(v);
    PRG_REQUIRE(k, PRG_ERR_STATE, "prg_fr_get_dualquats: set the skinning weights first");
    PRG_REQUIRE(k_nodes == k->K, PRG_ERR_INVALID, "prg_fr_get_dualquats: %d dual quaternions for %d nodes", k_nodes, k->K);
    PRG_ENTER(v.device);
    return prg::copy_out(dualquats_host, k->dq, (int64_t)k_nodes * 8, v.stream);
}

int prg_fr_kinematic_estep(prg_filterreg* h, double sigma2, double alpha, int* lattice_size, int* with_blur) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_fr_kinematic_estep: NULL argument");
    PRG_REQUIRE(sigma2 > 0.0, PRG_ERR_INVALID, "prg_fr_kinematic_estep: sigma2 must be > 0 (got %g)", sigma2);
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, false));
    Kin* k = kin_of(v);
    PRG_REQUIRE(k && v.have_src && v.have_tgt, PRG_ERR_STATE, "prg_fr_kinematic_estep: clouds or skinning weights not set");
    PRG_ENTER(v.device);
    k_kin_skin<<<(unsigned)prg::ceil_div(k->M, kBlock), kBlock, 0, v.stream>>>(v.src, k->ord_plan.p, k->kp.p, k->kw.p, k->dq.p, k->M, k->moved.p);
    PRG_HIP(hipGetLastError());
    // the embedding applies the plan's rigid state to what it is given: the identity here, the skinned cloud passes unchanged
    const double st13[13] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, sigma2};
    PRG_HIP(hipMemcpyAsync(v.state, st13, sizeof(st13), hipMemcpyHostToDevice, v.stream));
    PRG_HIP(hipStreamSynchronize(v.stream));
    k->use_arrays = false;
    k->have_normal = false;
    return prg::fr_estep_moved(h, k->moved.p, alpha, lattice_size, with_blur);
}

int prg_fr_kinematic_set_arrays(prg_filterreg* h, const double* t_source_hd, const float* m0_hd, const float* m1_hd,
                                const float* m2_hd, int64_t n_target) {
    PRG_REQUIRE(h && t_source_hd && m0_hd && m1_hd, PRG_ERR_INVALID, "prg_fr_kinematic_set_arrays: NULL argument");
    PRG_REQUIRE(n_target > 0, PRG_ERR_INVALID, "prg_fr_kinematic_set_arrays: need n_target > 0");
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, false));
    Kin* k = kin_of(v);
    PRG_REQUIRE(k, PRG_ERR_STATE, "prg_fr_kinematic_set_arrays: set the skinning weights first");
    PRG_ENTER(v.device);
    const size_t m = (size_t)k->M;
    // staging: t_source [m][3] f64 | m0 [m] | m1 [m][3] | m2 [m]
    const size_t o_m0 = m * 3 * sizeof(double), o_m1 = o_m0 + m * sizeof(float), o_m2 = o_m1 + m * 3 * sizeof(float),
                 total = o_m2 + m * sizeof(float);
    PRG_HIP(k->arrays.ensure((int64_t)total, (int64_t)total));
    char* a = k->arrays.p;
    PRG_HIP(hipMemcpyAsync(a, t_source_hd, m * 3 * sizeof(double), hipMemcpyDefault, v.stream));
    PRG_HIP(hipMemcpyAsync(a + o_m0, m0_hd, m * sizeof(float), hipMemcpyDefault, v.stream));
    PRG_HIP(hipMemcpyAsync(a + o_m1, m1_hd, m * 3 * sizeof(float), hipMemcpyDefault, v.stream));
    if (m2_hd) PRG_HIP(hipMemcpyAsync(a + o_m2, m2_hd, m * sizeof(float), hipMemcpyDefault, v.stream));
    PRG_HIP(hipStreamSynchronize(v.stream));
    k->arr_in = EstepIn{(const double*)a, 3, (const float*)(a + o_m0), 1, (const float*)(a + o_m1), 3,
                        m2_hd ? (const float*)(a + o_m2) : nullptr, 1};
    k->arr_n_target = n_target;
    k->use_arrays = true;
    k->have_normal = false;
    return PRG_OK;
}

int prg_fr_kinematic_normal_sums(prg_filterreg* h, double sigma2, double w, int reference_form, int n_segments,
                                 double* out_host) {
    PRG_REQUIRE(h && out_host, PRG_ERR_INVALID, "prg_fr_kinematic_normal_sums: NULL argument");
    PRG_REQUIRE(w >= 0.0 && w < 1.0, PRG_ERR_INVALID, "prg_fr_kinematic_normal_sums: w must be in [0, 1) (got %g)", w);
    PRG_REQUIRE(sigma2 > 0.0, PRG_ERR_INVALID, "prg_fr_kinematic_normal_sums: sigma2 must be > 0 (got %g)", sigma2);
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, true));
    Kin* k = kin_of(v);
    PRG_REQUIRE(k, PRG_ERR_STATE, "prg_fr_kinematic_normal_sums: set the skinning weights first");
    PRG_REQUIRE(k->use_arrays || v.have_estep, PRG_ERR_STATE, "prg_fr_kinematic_normal_sums: no E-step values");
    PRG_REQUIRE(n_segments == k->S, PRG_ERR_INVALID, "prg_fr_kinematic_normal_sums: %d segments expected, the plan has %d", n_segments, k->S);
    PRG_ENTER(v.device);
    EstepIn in = k->arr_in;
    const int* ord = k->ord_caller.p;
    int64_t n_target = k->arr_n_target;
    if (!k->use_arrays) {
        in = EstepIn{v.ts, 4, v.vout, v.ch, v.vout + 1, v.ch, v.vout + 4, v.ch};
        ord = k->ord_plan.p;
        n_target = v.N;
    }
    const double c = w / (1.0 - w) * (double)n_target / (double)k->M;  // filterreg.py:222 (no (2 pi sigma2)^(3/2), sic)
    k_kin_normal<<<k->n_chunks, kBlock, 0, v.stream>>>(k->chunks.p, ord, in, k->kw.p, c, sigma2, reference_form, k->pt.p, k->mu.p, k->part.p);
    PRG_HIP(hipGetLastError());
    k->have_normal = true;
    return seg_sums_to_host(k, kNrm, v.stream, out_host);
}

int prg_fr_kinematic_grad_sums(prg_filterreg* h, const double* twists_host, int reference_form, int n_segments,
                               double* out_host) {
    PRG_REQUIRE(h && twists_host && out_host, PRG_ERR_INVALID, "prg_fr_kinematic_grad_sums: NULL argument");
    prg::FrView v;
    PRG_TRY(prg::fr_view(h, &v, false));
    Kin* k = kin_of(v);
    PRG_REQUIRE(k && k->have_normal, PRG_ERR_STATE, "prg_fr_kinematic_grad_sums: run prg_fr_kinematic_normal_sums first");
    PRG_REQUIRE(n_segments == k->S, PRG_ERR_INVALID, "prg_fr_kinematic_grad_sums: %d segments expected, the plan has %d", n_segments, k->S);
    PRG_ENTER(v.device);
    PRG_HIP(hipMemcpyAsync(k->tw.p, twists_host, (size_t)k->K * 6 * sizeof(double), hipMemcpyHostToDevice, v.stream));
    k_dq_from_twist<<<(unsigned)prg::ceil_div(k->K, 64), 64, 0, v.stream>>>(k->tw.p, k->K, k->dq_inc.p);
    k_kin_grad<<<k->n_chunks, kBlock, 0, v.stream>>>(k->chunks.p, k->pt.p, k->mu.p, k->kp.p, k->kw.p, k->dq_inc.p, reference_form, k->part.p);
    PRG_HIP(hipGetLastError());
    return seg_sums_to_host(k, kGrd, v.stream, out_host);
}

int prg_fr_kinematic_sums_from_arrays(int device, void* hip_stream, const double* t_source_hd, int64_t m,
                                      int64_t n_target, const float* m0_hd, const float* m1_hd, const float* m2_hd,
                                      const int* pairs_hd, const float* weights_hd, int k_nodes, double sigma2, double w,
                                      int reference_form, const double* twists_host, int n_segments,
                                      double* normal_out_host, double* grad_out_host) {
    PRG_REQUIRE(t_source_hd && normal_out_host && grad_out_host, PRG_ERR_INVALID, "prg_fr_kinematic_sums_from_arrays: NULL argument");
    PRG_REQUIRE(k_nodes > 0, PRG_ERR_INVALID, "prg_fr_kinematic_sums_from_arrays: need k_nodes > 0");
    prg_filterreg* h = nullptr;
    PRG_TRY(prg_fr_create(&h, device, hip_stream));
    int n_seg = 0;
    int st = prg_fr_set_source(h, t_source_hd, m, 3);
    if (st == PRG_OK) st = prg_fr_set_skinning(h, pairs_hd, weights_hd, m, k_nodes, &n_seg);
    if (st == PRG_OK) st = prg_fr_kinematic_set_arrays(h, t_source_hd, m0_hd, m1_hd, m2_hd, n_target);
    if (st == PRG_OK) st = prg_fr_kinematic_normal_sums(h, sigma2, w, reference_form, n_segments, normal_out_host);
    if (st == PRG_OK) {
        std::vector<double> zero((size_t)k_nodes * 6, 0.0);
        st = prg_fr_kinematic_grad_sums(h, twists_host ? twists_host : zero.data(), reference_form, n_segments, grad_out_host);
    }
    (void)prg_fr_destroy(h);
    return st;
}

}  // extern "C"
