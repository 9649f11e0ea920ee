// Kernel-field evaluation (prg_field_*): f(x)_c = sum_m k(|x - y_m|^2) w_mc for any query points x, the continuous displacement
// field behind the non-rigid results (Gaussian of non-rigid CPD, inverse multiquadric of BCPD, thin-plate spline of GMMReg).
// DESIGN.md section 3.18 is the definition: fp64 throughout, control points in ascending index, slabs of 65 536 control points
// whose sums are added in ascending order, no floating-point atomics; a result does not depend on Q, on the launch geometry
// or on how the queries are batched.
#include <math.h>

#include <algorithm>

#include "prg_common.h"

namespace {

constexpr int kBlock = 64;                  // one wave; a lane owns kPerLane queries
constexpr int kPerLane = 2;                 // two fp64 exp / log / rsqrt chains per lane hide each other's latency
constexpr int kTile = kBlock * kPerLane;    // queries of a block
constexpr int kUnroll = 4;                  // control points per trip of the slab loop
constexpr int64_t kSlab = 65536;            // control points per slab: a constant of the definition
constexpr int64_t kPartBytes = 64ll << 20;  // the slab-partial buffer never grows past this
constexpr int kPackBlock = 256;

enum { kGaussian = 0, kImq = 1, kTps2 = 2, kTps3 = 3 };

// 1 / sqrt(d) for d > 0 to ~1 ulp: v_rsq_f64 (2^-26) and two Newton-Raphson steps (as the Cholesky of spd_solve.hip takes it)
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = fma(-d * y, y, 1.0);  // 1 - d y^2
        y = fma(0.5 * y, e, y);
    }
    return y;
}

// k(d2).  gaussian: p0 + p1 = -1 / (2 beta) to twice the precision of a double, so the argument is d2 / (2 beta) rounded once
// (within 2^-105 of it) without a division per pair; imq: p0 = c.
template <int KIND>
__device__ __forceinline__ double kernel_of(double d2, double p0, double p1) {
    if (KIND == kGaussian) return exp(fma(d2, p0, d2 * p1));
    if (KIND == kImq) return rsqrt_nr(d2 + p0);
    if (KIND == kTps2) return d2 > 1.0e-9 ? 0.5 * d2 * log(d2) : 0.0;
    return -sqrt(d2);
}

// rows: [m_pad][3 + C] doubles (y_x, y_y, y_z, w_0 .. w_{C-1}), m_pad a multiple of kUnroll, pad rows with the coordinates of
// control point 0 and zero weights (k is finite there and acc + 0 k = acc), z = 0 for D = 2 on both sides.  Block (bx, by):
// queries [bx kTile, (bx + 1) kTile) of the nq at `pts`, slab by.  dst[(by nq + q) C + c]: the output itself when there is one
// slab, else the slab-partial buffer.  The row addresses are wave-uniform, so rows arrive through scalar loads.
template <int KIND, int C>
__global__ __launch_bounds__(kBlock) void k_field(const double* __restrict__ rows, int64_t m_pad,
                                                  const double* __restrict__ pts, int64_t nq, int dim, double p0, double p1,
                                                  double* __restrict__ dst) {
    constexpr int R = 3 + C;
    const int64_t q0 = (int64_t)blockIdx.x * kTile + threadIdx.x;
    double x[kPerLane][3], acc[kPerLane][C];
#pragma unroll
    for (int t = 0; t < kPerLane; ++t) {
        const int64_t q = q0 + (int64_t)t * kBlock;
        const bool in = q < nq;  // (a lane without a query computes on the origin and stores nothing)
        x[t][0] = in ? pts[q * dim] : 0.0;
        x[t][1] = in ? pts[q * dim + 1] : 0.0;
        x[t][2] = in && dim > 2 ? pts[q * dim + 2] : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[t][c] = 0.0;
    }
    const int64_t j0 = (int64_t)blockIdx.y * kSlab;
    const int64_t j1 = j0 + kSlab < m_pad ? j0 + kSlab : m_pad;
    for (int64_t j = j0; j < j1; j += kUnroll) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const double* __restrict__ r = rows + (j + u) * R;
            const double y0 = r[0], y1 = r[1], y2 = r[2];
#pragma unroll
            for (int t = 0; t < kPerLane; ++t) {
                const double dx = x[t][0] - y0, dy = x[t][1] - y1, dz = x[t][2] - y2;
                const double k = kernel_of<KIND>(fma(dz, dz, fma(dy, dy, dx * dx)), p0, p1);
#pragma unroll
                for (int c = 0; c < C; ++c) acc[t][c] = fma(k, r[3 + c], acc[t][c]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kPerLane; ++t) {
        const int64_t q = q0 + (int64_t)t * kBlock;
        if (q < nq) {
#pragma unroll
            for (int c = 0; c < C; ++c) dst[((int64_t)blockIdx.y * nq + q) * C + c] = acc[t][c];
        }
    }
}

// out[i] = part[0][i] + part[1][i] + ... in ascending slab order; i over the nq C outputs of a batch
__global__ __launch_bounds__(kPackBlock) void k_field_add_slabs(const double* __restrict__ part, int64_t count, int nslabs,
                                                                double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
    if (i >= count) return;
    double s = part[i];
    for (int k = 1; k < nslabs; ++k) s += part[(int64_t)k * count + i];
    out[i] = s;
}

__global__ __launch_bounds__(kPackBlock) void k_field_pack(const double* __restrict__ control, const double* __restrict__ w,
                                                           int64_t m, int64_t m_pad, int dim, int C,
                                                           double* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * kPackBlock + threadIdx.x;
    if (i >= m_pad) return;
    const int64_t src = i < m ? i : 0;
    double* r = rows + i * (3 + C);
    r[0] = control[src * dim];
    r[1] = control[src * dim + 1];
    r[2] = dim > 2 ? control[src * dim + 2] : 0.0;
    for (int c = 0; c < C; ++c) r[3 + c] = i < m ? w[i * C + c] : 0.0;
}

template <int KIND>
void launch_kind(int C, dim3 grid, hipStream_t st, const double* rows, int64_t m_pad, const double* pts, int64_t nq, int dim,
                 double p0, double p1, double* dst) {
    switch (C) {
        case 1: k_field<KIND, 1><<<grid, kBlock, 0, st>>>(rows, m_pad, pts, nq, dim, p0, p1, dst); break;
        case 2: k_field<KIND, 2><<<grid, kBlock, 0, st>>>(rows, m_pad, pts, nq, dim, p0, p1, dst); break;
        case 3: k_field<KIND, 3><<<grid, kBlock, 0, st>>>(rows, m_pad, pts, nq, dim, p0, p1, dst); break;
        default: k_field<KIND, 4><<<grid, kBlock, 0, st>>>(rows, m_pad, pts, nq, dim, p0, p1, dst); break;
    }
}

}  // namespace

struct prg_field {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t M = 0, m_pad = 0;  // M == 0: no control points yet
    int D = 0, C = 0, kind = 0;
    double p0 = 0.0, p1 = 0.0;
    prg::DevBuf<double> rows;        // [m_pad][3 + C]
    prg::DevBuf<double> stage;       // the caller's arrays as they came: control and weights, later the queries
    prg::DevBuf<double> out, part;   // [Q][C], [nslabs][batch][C]
};

extern "C" {

int prg_field_create(prg_field** out, int device, void* hip_stream) {
    return prg::create_handle(__func__, out, device, hip_stream);
}

int prg_field_destroy(prg_field* h) {
    return prg::destroy_handle(h);
}

int prg_field_set_control(prg_field* h, const double* control_hd, const double* weights_hd, int64_t m, int d, int c, int kind,
                          double param) {
    PRG_REQUIRE(d == 2 || d == 3, PRG_ERR_INVALID, "prg_field_set_control: d must be 2 or 3, got %d", d);
    PRG_REQUIRE(c >= 1 && c <= 4, PRG_ERR_INVALID, "prg_field_set_control: c must lie in 1 .. 4, got %d", c);
    PRG_REQUIRE(kind >= PRG_FIELD_GAUSSIAN && kind <= PRG_FIELD_TPS, PRG_ERR_INVALID,
                "prg_field_set_control: kind must be 0 (gaussian), 1 (imq) or 2 (tps), got %d", kind);
    PRG_REQUIRE(kind == PRG_FIELD_TPS || (std::isfinite(param) && param > 0.0), PRG_ERR_INVALID,
                "prg_field_set_control: %s must be finite and > 0, got %g", kind == PRG_FIELD_GAUSSIAN ? "beta" : "c", param);
    PRG_REQUIRE(m >= 1 && m < (int64_t)1 << 31, PRG_ERR_INVALID,
                "prg_field_set_control: need 1 <= m < 2^31 control points, got %lld", (long long)m);
    PRG_REQUIRE(h && control_hd && weights_hd, PRG_ERR_INVALID, "prg_field_set_control: NULL argument");
    PRG_ENTER(h->device);
    h->M = 0;
    const int64_t m_pad = prg::ceil_div(m, kUnroll) * kUnroll;
    PRG_HIP(hipStreamSynchronize(h->stream));  // (a buffer that grows is freed: nothing may still read it)
    PRG_HIP(h->rows.ensure(m_pad * (3 + c), m_pad * (3 + c)));
    PRG_HIP(h->stage.ensure(m * (d + c), m * (d + c)));
    PRG_TRY(prg::copy_in(h->stage, control_hd, m * d, h->stream));
    PRG_TRY(prg::copy_in(h->stage, weights_hd, m * c, h->stream, m * d));
    k_field_pack<<<(unsigned)prg::ceil_div(m_pad, kPackBlock), kPackBlock, 0, h->stream>>>(h->stage.p, h->stage.p + m * d, m,
                                                                                           m_pad, d, c, h->rows.p);
    PRG_HIP(hipGetLastError());
    if (kind == PRG_FIELD_GAUSSIAN) {
        // -1 / (2 beta) as p0 + p1: p0 the rounded quotient, p1 its remainder (1 + p0 2 beta is exact in an fma)
        const double tb = 2.0 * param;
        h->p0 = -1.0 / tb;
        h->p1 = -fma(h->p0, tb, 1.0) / tb;
    } else {
        h->p0 = param;
        h->p1 = 0.0;
    }
    h->kind = kind == PRG_FIELD_TPS ? (d == 2 ? kTps2 : kTps3) : kind;
    h->D = d;
    h->C = c;
    h->m_pad = m_pad;
    h->M = m;
    return PRG_OK;
}

int prg_field_evaluate(prg_field* h, const double* points_hd, int64_t q, double* out_host) {
    PRG_REQUIRE(q >= 0 && q < (int64_t)1 << 31, PRG_ERR_INVALID, "prg_field_evaluate: need 0 <= q < 2^31 queries, got %lld",
                (long long)q);
    PRG_REQUIRE(h != nullptr, PRG_ERR_INVALID, "prg_field_evaluate: NULL argument");
    PRG_REQUIRE(h->M >= 1, PRG_ERR_STATE, "prg_field_evaluate: no control points (prg_field_set_control first)");
    if (q == 0) return PRG_OK;
    PRG_REQUIRE(points_hd && out_host, PRG_ERR_INVALID, "prg_field_evaluate: NULL argument");
    PRG_ENTER(h->device);
    hipStream_t st = h->stream;
    const int D = h->D, C = h->C;
    const int nslabs = (int)prg::ceil_div(h->m_pad, kSlab);
    // queries per launch: everything when the kernel writes the output itself, else what keeps [nslabs][batch][C] bounded
    int64_t batch = q;
    if (nslabs > 1) {
        batch = std::max<int64_t>(kPartBytes / ((int64_t)sizeof(double) * C * nslabs) / kTile, 1) * kTile;
        batch = std::min(batch, q);
    }
    PRG_HIP(hipStreamSynchronize(st));
    PRG_HIP(h->stage.ensure(q * D, q * D));
    PRG_HIP(h->out.ensure(q * C, q * C));
    if (nslabs > 1) PRG_HIP(h->part.ensure(batch * C * nslabs, batch * C * nslabs));
    PRG_TRY(prg::copy_in(h->stage, points_hd, q * D, st));
    for (int64_t first = 0; first < q; first += batch) {
        const int64_t nq = std::min(batch, q - first);
        const dim3 grid((unsigned)prg::ceil_div(nq, kTile), (unsigned)nslabs);
        const double* pts = h->stage.p + first * D;
        double* dst = nslabs > 1 ? h->part.p : h->out.p + first * C;
        switch (h->kind) {
            case kGaussian: launch_kind<kGaussian>(C, grid, st, h->rows.p, h->m_pad, pts, nq, D, h->p0, h->p1, dst); break;
            case kImq: launch_kind<kImq>(C, grid, st, h->rows.p, h->m_pad, pts, nq, D, h->p0, h->p1, dst); break;
            case kTps2: launch_kind<kTps2>(C, grid, st, h->rows.p, h->m_pad, pts, nq, D, h->p0, h->p1, dst); break;
            default: launch_kind<kTps3>(C, grid, st, h->rows.p, h->m_pad, pts, nq, D, h->p0, h->p1, dst); break;
        }
        if (nslabs > 1)
            k_field_add_slabs<<<(unsigned)prg::ceil_div(nq * C, kPackBlock), kPackBlock, 0, st>>>(h->part.p, nq * C, nslabs,
                                                                                                 h->out.p + first * C);
        PRG_HIP(hipGetLastError());
    }
    return prg::copy_out(out_host, h->out, q * C, st);
}

}  // extern "C"
