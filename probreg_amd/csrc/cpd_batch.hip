// The CPD batch plan for MI355X (gfx950): B independent rigid / affine registrations of small clouds run with a launch count that
// does not depend on B.  One EM iteration of the WHOLE batch is two launches:
//   k_batch_sweep   one workgroup per tile of kBatchTile target columns of one problem (host-built tile table).  The workgroup
//                   transforms its problem's source itself, kBatchChunk points at a time through LDS, from the problem's parameter
//                   block; every lane owns one column and keeps (min d^2, A, U, R) under the online rescaling of the residual
//                   column form (algebra in k_colpass_cull<true> / k_colfinal_resid); the column's share of the
//                   M-step's moments is formed in fp64 and the workgroup writes ONE fp64 partial per tile.
//   k_batch_mstep   one workgroup per problem: tile partials summed in a fixed order, the z-side sums mapped back to the source's
//                   frame, the M-step of k_mstep (prg::mstep_body, cpd_mstep.h), the convergence test of cpd.py:115-117 against
//                   the problem's own tolerance, the done flag, n_iter and the count of problems still running.
// A problem that is done is frozen: its tiles and its M-step return at once.  Workgroups talk only through kernel boundaries: no
// grid-wide barrier, no spin on another workgroup's memory, no cooperative launch, no floating-point atomics; every loop bound is a
// kernel argument or an entry of the (constant) offset tables.  Sums run in a fixed order and a tile depends on its own problem's
// (M_b, N_b) only, so a problem's result does not depend on what else is in the batch, or where.
//
// Reference behaviour (neka-nat/probreg v0.3.7): the EM driver cpd.py:106-120, E-step cpd.py:71-88, M-steps cpd.py:160-192 and
// 219-244, initialisation cpd.py:145-153 / 209-217 with math_utils.py:28-29 in closed form.
#include <math.h>

#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "cpd_mstep.h"
#include "cpd_sweeps.h"
#include "prg_common.h"
#include "prg_device.h"

struct prg_cpd_batch {
    int device = 0;
    hipStream_t stream = nullptr;
    int dim = 3, B = 0, ntiles = 0;
    int64_t Mtot = 0, Ntot = 0;
    prg::DevBuf<float4> src4;     // [Mtot] centred source points (fp32, as the single plan uploads them)
    prg::DevBuf<float4> tgt4;     // [Ntot]
    prg::DevBuf<int64_t> soff;    // [B + 1] first source point of every problem
    prg::DevBuf<int64_t> toff;    // [B + 1]
    prg::DevBuf<int4> tiles;      // [ntiles] (problem, first column, column count, 0)
    prg::DevBuf<int> tile_first;  // [B + 1] first tile of every problem
    prg::DevBuf<double> params;   // [B][PRG_NPARAMS]
    prg::DevBuf<double> part;     // [ntiles][kBatchComp]
    prg::DevBuf<double> init;     // [B][16]
    prg::DevBuf<double> wtol;     // [2][B]: w, tol
    prg::DevBuf<int> flags;       // done[B], n_iter[B], active
    prg::HostBuf<double> pinned;  // host staging: 2 B doubles (w, tol), then one int (active) in 8 more
    std::vector<double> wtol_host;  // what wtol holds (w, tol of the last prg_cpd_batch_iterate)
    bool initialised = false;
};

namespace {
constexpr int kBatchTile = 128;   // target columns per tile = threads per sweep workgroup (one column per lane)
constexpr int kBatchChunk = 128;  // source points transformed into LDS per trip (one per thread)
constexpr int kBatchComp = 24;    // doubles per tile partial: MOMENTS [0..23] of probreg_hip.h, z-side sums still in the moved frame
constexpr int kPoll = 8;          // EM iterations enqueued between two reads of the active counter
constexpr double kLog2e = 1.4426950408889634;

// ---------------------------------------------------------------------------------------------------------------------------------
// One workgroup per problem: cloud sums, sigma2_0 and q_0 - the algebra of k_init_params (cpd.hip) for every problem at once.
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_batch_init(const float4* __restrict__ src4, const float4* __restrict__ tgt4,
                                                    const int64_t* __restrict__ soff, const int64_t* __restrict__ toff,
                                                    const double* __restrict__ init /* [B][16] or null */,
                                                    double* __restrict__ params, int* __restrict__ flags, int nb, int dim) {
    __shared__ double sh[4][8];
    const int b = blockIdx.x;
    const int64_t s0 = soff[b], m = soff[b + 1] - s0, t0 = toff[b], n = toff[b + 1] - t0;
    double a[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // source: sum y, sum |y|^2 ; target: sum x, sum |x|^2
    for (int64_t i = threadIdx.x; i < m; i += 256) {
        const float4 v = src4[s0 + i];
        a[0] += v.x; a[1] += v.y; a[2] += v.z;
        a[3] += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z;
    }
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float4 v = tgt4[t0 + i];
        a[4] += v.x; a[5] += v.y; a[6] += v.z;
        a[7] += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double s = wave_sum(a[c]);
        if (lane == 0) sh[wv][c] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double ss[4], ts[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ss[c] = sh[0][c] + sh[1][c] + sh[2][c] + sh[3][c];
        ts[c] = sh[0][4 + c] + sh[1][4 + c] + sh[2][4 + c] + sh[3][4 + c];
    }
    const double dm = (double)m, dn = (double)n;
    // sigma2_0 = [M sum|x|^2 + N sum|y|^2 - 2 (sum x).(sum y)] / (D M N)   (math_utils.py:28-29 in closed form)
    double total = dm * ts[3] + dn * ss[3] - 2.0 * (ts[0] * ss[0] + ts[1] * ss[1] + ts[2] * ss[2]);
    const double* ib = init ? init + (int64_t)b * 16 : nullptr;
    if (ib) {
        // the two clouds were centred on different origins (delta = origin_target - origin_source), as in k_init_params:
        // sum |x' - y' + delta|^2 = sum |x' - y'|^2 + 2 delta.(M sum x' - N sum y') + M N |delta|^2
        double lin = 0.0, d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lin += ib[13 + k] * (dm * ts[k] - dn * ss[k]);
            d2 += ib[13 + k] * ib[13 + k];
        }
        total += 2.0 * lin + dm * dn * d2;
    }
    const double sigma2 = total / (dim * dm * dn);
    double* p = params + (int64_t)b * PRG_NPARAMS;
    for (int i = 0; i < PRG_NPARAMS; ++i) p[i] = 0.0;
    if (ib) {
        for (int i = 0; i < 13; ++i) p[i] = ib[i];
    } else {
        p[0] = p[4] = p[8] = 1.0;
        p[12] = 1.0;
    }
    p[13] = sigma2;
    p[14] = 1.0 + dn * dim * 0.5 * log(sigma2);  // cpd.py:148
    flags[b] = 0;                                // done
    flags[nb + b] = 0;                           // n_iter
    if (b == 0) flags[2 * nb] = nb;              // problems still running
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The ragged pair sweep.  Per column: run = min_m d^2 so far, off = prg::col_offset(kk, run), K = exp2(kk d^2 + off) <= 1,
//   A = sum K,  U = sum K (x - z),  R = sum K |x - z|^2        (AFFINE: V = sum K y y^T, six channels, y the source's own point)
// all moved to the new offset whenever the minimum drops.  K is exactly 0 below 2^-126 of the column's largest term; nothing else is
// dropped (the 2^-48 bound of the culled sweeps is the accepted truncation, and this sweep does not even cull).  The column's
// normaliser is rebuilt in fp64, den = A 2^-off: a column whose every term underflows fp32 but not fp64 keeps its full weight, and
// cpd.py:81's den == 0 -> eps32 (an all-zero column of P) applies exactly where the fp64 reference has it.
// Moment terms per column (fp64, x_n the origin; k_colfinal_resid): sum_m K z = x A - U, sum_m K |z|^2 = |x|^2 A - 2 x.U + R:
//   [0] pt1  [1..3] pt1 x  [4..6] pz = pt1 x - q U  [7..15] x pz^T  [22] pt1 |x|^2,  q = pt1 / A
//   rigid:  [16] pt1 |x|^2 + q (R - 2 x.U)  (trace of the z-side second moment; k_batch_mstep maps it back)
//   affine: [16..21] q V  (Y^T diag(p1) Y itself: the weights carry all of its error, and a source that lies in a plane keeps
//           its exact zero row, which is what the M-step's singularity test looks at)
// ---------------------------------------------------------------------------------------------------------------------------------
template <bool AFFINE>
__global__ __launch_bounds__(kBatchTile) void k_batch_sweep(const int4* __restrict__ tiles, const float4* __restrict__ src4,
                                                            const float4* __restrict__ tgt4, const int64_t* __restrict__ soff,
                                                            const int64_t* __restrict__ toff, const double* __restrict__ params,
                                                            const int* __restrict__ done, const double* __restrict__ wv,
                                                            double* __restrict__ part, int dim) {
    __shared__ float4 zs[kBatchChunk];
    __shared__ float4 ya[AFFINE ? kBatchChunk : 1];  // yy (xx, xy, xz, yy)
    __shared__ float2 yb[AFFINE ? kBatchChunk : 1];  // yy (yz, zz)
    __shared__ double sh[2][kBatchComp];
    const int4 tile = tiles[blockIdx.x];
    const int b = tile.x;
    if (done[b]) return;  // (workgroup-uniform: before any barrier)
    const double* __restrict__ P = params + (int64_t)b * PRG_NPARAMS;
    const double L00 = P[0], L01 = P[1], L02 = P[2], L10 = P[3], L11 = P[4], L12 = P[5], L20 = P[6], L21 = P[7], L22 = P[8];
    const double t0 = P[9], t1 = P[10], t2 = P[11], sc = P[12], sigma2 = P[13];
    const float kk = (float)(-kLog2e / (2.0 * sigma2));
    const int64_t s0 = soff[b], t_first = toff[b];
    const int m = (int)(soff[b + 1] - s0);
    const int n = (int)(toff[b + 1] - t_first);
    const bool valid = (int)threadIdx.x < tile.z;
    // lanes past the end of the tile redo its last column and contribute nothing: the wave stays whole
    const float4 xf = tgt4[t_first + tile.y + (valid ? (int)threadIdx.x : tile.z - 1)];
    float run = INFINITY, off = INFINITY;
    float A = 0.f, U0 = 0.f, U1 = 0.f, U2 = 0.f, R = 0.f;
    float V0 = 0.f, V1 = 0.f, V2 = 0.f, V3 = 0.f, V4 = 0.f, V5 = 0.f;
    for (int c0 = 0; c0 < m; c0 += kBatchChunk) {
        __syncthreads();  // the previous chunk has been consumed
        {
            float4 z = make_float4(prg::kSrcPad, prg::kSrcPad, prg::kSrcPad, 0.f);  // a pad is 1e18 away: K == 0
            float4 qa = make_float4(0.f, 0.f, 0.f, 0.f);
            float2 qb = make_float2(0.f, 0.f);
            if (c0 + (int)threadIdx.x < m) {
                const float4 y = src4[s0 + c0 + threadIdx.x];
                const double y0 = y.x, y1 = y.y, y2 = y.z;
                z.x = (float)(sc * (L00 * y0 + L01 * y1 + L02 * y2) + t0);  // transformation.py:49-50 / 77-78
                z.y = (float)(sc * (L10 * y0 + L11 * y1 + L12 * y2) + t1);
                z.z = dim > 2 ? (float)(sc * (L20 * y0 + L21 * y1 + L22 * y2) + t2) : 0.f;
                if (AFFINE) {
                    qa = make_float4(y.x * y.x, y.x * y.y, y.x * y.z, y.y * y.y);
                    qb = make_float2(y.y * y.z, y.z * y.z);
                }
            }
            zs[threadIdx.x] = z;
            if (AFFINE) {
                ya[threadIdx.x] = qa;
                yb[threadIdx.x] = qb;
            }
        }
        __syncthreads();
        const int left = m - c0;
        const int cnt = left < kBatchChunk ? ((left + 3) & ~3) : kBatchChunk;  // (the pads fill the last quad)
        for (int g = 0; g < cnt; g += 4) {
            float dx[4], dy[4], dz[4], d2[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float4 z = zs[g + c];
                dx[c] = xf.x - z.x;
                dy[c] = xf.y - z.y;
                dz[c] = xf.z - z.z;
                d2[c] = fmaf(dz[c], dz[c], fmaf(dy[c], dy[c], dx[c] * dx[c]));
            }
            const float cm = fminf(fminf(d2[0], d2[1]), fminf(d2[2], d2[3]));
            if (cm < run) {  // rare after the first trips: every sum moves to the new minimum's offset
                const float noff = prg::col_offset(kk, cm);
                const float f = __builtin_amdgcn_exp2f(noff - off);  // first use: off == +inf -> 0, and the sums are 0 anyway
                A *= f; U0 *= f; U1 *= f; U2 *= f; R *= f;
                if (AFFINE) { V0 *= f; V1 *= f; V2 *= f; V3 *= f; V4 *= f; V5 *= f; }
                run = cm;
                off = noff;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float pr = __builtin_amdgcn_exp2f(fmaf(d2[c], kk, off));
                A += pr;
                U0 = fmaf(pr, dx[c], U0);
                U1 = fmaf(pr, dy[c], U1);
                U2 = fmaf(pr, dz[c], U2);
                R = fmaf(pr, d2[c], R);
                if (AFFINE) {
                    const float4 qa = ya[g + c];
                    const float2 qb = yb[g + c];
                    V0 = fmaf(pr, qa.x, V0);
                    V1 = fmaf(pr, qa.y, V1);
                    V2 = fmaf(pr, qa.z, V2);
                    V3 = fmaf(pr, qa.w, V3);
                    V4 = fmaf(pr, qb.x, V4);
                    V5 = fmaf(pr, qb.y, V5);
                }
            }
        }
    }
    // ---- the column's normaliser and its moment terms, fp64 (k_colfinal_resid) ----
    const double w = wv[b];
    const double Ad = (double)A;
    const double den = Ad * exp2(-(double)off);  // underflows to 0 exactly where fp64 exp() does
    double c = 0.0;
    if (w > 0.0) c = pow(2.0 * M_PI * sigma2, dim * 0.5) * (w / (1.0 - w) * ((double)m / (double)n));  // cpd.py:76-77
    double a[kBatchComp];
#pragma unroll
    for (int k = 0; k < kBatchComp; ++k) a[k] = 0.0;
    if (valid && den != 0.0) {  // den == 0: cpd.py:81 sets eps32 and the column of P is all zero
        const double pd = den / (den + c), qn = pd / Ad;
        const double x[3] = {xf.x, xf.y, xf.z};
        const double U[3] = {U0, U1, U2};
        double pz[3], xu = 0.0, xx = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pz[k] = pd * x[k] - qn * U[k];
            xu += x[k] * U[k];
            xx += x[k] * x[k];
        }
        a[0] = pd;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            a[1 + r] = pd * x[r];
            a[4 + r] = pz[r];
#pragma unroll
            for (int k = 0; k < 3; ++k) a[7 + 3 * r + k] = x[r] * pz[k];
        }
        if (AFFINE) {
            a[16] = qn * (double)V0; a[17] = qn * (double)V1; a[18] = qn * (double)V2;
            a[19] = qn * (double)V3; a[20] = qn * (double)V4; a[21] = qn * (double)V5;
        } else {
            a[16] = pd * xx + qn * ((double)R - 2.0 * xu);
        }
        a[22] = pd * xx;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kBatchComp; ++k) {
        const double s = wave_sum(a[k]);
        if (lane == 0) sh[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kBatchComp) part[(int64_t)blockIdx.x * kBatchComp + threadIdx.x] = sh[0][threadIdx.x] + sh[1][threadIdx.x];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// One workgroup per problem.  The sweep saw the TRANSFORMED source z = s L y + t; the M-step wants sums over y = G (z - t) with
// G = (s L)^-1 (rigid: L^T / s, L a rotation; affine: the inverse of b):
//   Sy = G (Sz - S0 t),  Sxy = (Sxz - Sx t^T) G^T,  rigid: tr Syy = (tr Szz - 2 t.Sz + S0 |t|^2) / s^2   (k_fused_final)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_batch_mstep(const double* __restrict__ part, const int* __restrict__ tile_first,
                                                    double* __restrict__ params, int* __restrict__ flags,
                                                    const double* __restrict__ tolv, int nb, int kind, int update_scale,
                                                    int dim) {
    __shared__ double m[PRG_NMOMENTS], mom[PRG_NMOMENTS];
    const int b = blockIdx.x;
    if (flags[b]) return;  // done: frozen
    if (threadIdx.x < PRG_NMOMENTS) {
        double s = 0.0;
        if (threadIdx.x < kBatchComp)
            for (int t = tile_first[b]; t < tile_first[b + 1]; ++t) s += part[(int64_t)t * kBatchComp + threadIdx.x];
        m[threadIdx.x] = s;
        mom[threadIdx.x] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double* __restrict__ P = params + (int64_t)b * PRG_NPARAMS;
    const double S0 = m[0], s = P[12];
    const double t[3] = {P[9], P[10], P[11]};
    double G[3][3];
    if (kind == PRG_TF_RIGID) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) G[j][k] = P[3 * k + j] / s;
    } else {
        const double b00 = P[0], b01 = P[1], b02 = P[2], b10 = P[3], b11 = P[4], b12 = P[5], b20 = P[6], b21 = P[7], b22 = P[8];
        const double c00 = b11 * b22 - b12 * b21, c01 = b12 * b20 - b10 * b22, c02 = b10 * b21 - b11 * b20;
        const double idet = 1.0 / (b00 * c00 + b01 * c01 + b02 * c02);
        G[0][0] = c00 * idet; G[0][1] = (b02 * b21 - b01 * b22) * idet; G[0][2] = (b01 * b12 - b02 * b11) * idet;
        G[1][0] = c01 * idet; G[1][1] = (b00 * b22 - b02 * b20) * idet; G[1][2] = (b02 * b10 - b00 * b12) * idet;
        G[2][0] = c02 * idet; G[2][1] = (b01 * b20 - b00 * b21) * idet; G[2][2] = (b00 * b11 - b01 * b10) * idet;
    }
    double tsz = 0.0, tt = 0.0;
    mom[0] = S0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        mom[1 + i] = m[1 + i];
        tsz += t[i] * m[4 + i];
        tt += t[i] * t[i];
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double sy = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) sy += G[j][k] * (m[4 + k] - S0 * t[k]);
        mom[4 + j] = sy;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) v += (m[7 + 3 * i + k] - m[1 + i] * t[k]) * G[j][k];
            mom[7 + 3 * i + j] = v;
        }
    if (kind == PRG_TF_RIGID) {
        mom[16] = (m[16] - 2.0 * tsz + S0 * tt) / (s * s);  // (the rigid fit takes the trace only, cpd.py:179-182; [17..21] stay 0)
    } else {
#pragma unroll
        for (int k = 16; k < 22; ++k) mom[k] = m[k];
    }
    mom[22] = m[22];
    const double q_prev = P[14];
    prg::mstep_body(mom, P, kind, update_scale, dim);
    const double q = P[14];
    const int it = flags[nb + b] + 1;
    flags[nb + b] = it;
    // cpd.py:115-117: stop when |q - q_prev| < tol and keep this M-step's state (tol < 0: never).  A fit that is no longer finite
    // (singular affine system) stops too: the host turns it into LinAlgError
    const bool finite = fabs(q) <= 1.0e300;
    if (fabs(q - q_prev) < tolv[b] || !finite) {
        flags[b] = 1;
        atomicSub(flags + 2 * nb, 1);
    }
}

int check_sizes(const char* who, int nb, const int64_t* m, const int64_t* n) {
    PRG_REQUIRE(nb > 0 && m && n, PRG_ERR_INVALID, "%s: need B > 0 and both size tables", who);
    for (int b = 0; b < nb; ++b)
        PRG_REQUIRE(m[b] > 0 && n[b] > 0 && m[b] < (1ll << 30) && n[b] < (1ll << 30), PRG_ERR_INVALID,
                    "%s: problem %d has %lld source and %lld target points (need 1 .. 2^30 - 1 each)", who, b, (long long)m[b],
                    (long long)n[b]);
    return PRG_OK;
}
}  // namespace

extern "C" {

int prg_cpd_batch_tile_shape(int* tile_columns, int* source_chunk) {
    PRG_REQUIRE(tile_columns && source_chunk, PRG_ERR_INVALID, "prg_cpd_batch_tile_shape: NULL argument");
    *tile_columns = kBatchTile;
    *source_chunk = kBatchChunk;
    return PRG_OK;
}

int prg_cpd_batch_tile_table(int nb, const int64_t* m, const int64_t* n, int* tiles_out, int64_t capacity, int64_t* ntiles) {
    PRG_TRY(check_sizes("prg_cpd_batch_tile_table", nb, m, n));
    PRG_REQUIRE(ntiles, PRG_ERR_INVALID, "prg_cpd_batch_tile_table: NULL argument");
    int64_t count = 0;
    for (int b = 0; b < nb; ++b)  // (the tile rule: kBatchTile columns each, the last one what is left - a function of N_b alone)
        for (int64_t c = 0; c < n[b]; c += kBatchTile, ++count)
            if (tiles_out && count < capacity) {
                tiles_out[3 * count] = b;
                tiles_out[3 * count + 1] = (int)c;
                tiles_out[3 * count + 2] = (int)(n[b] - c < kBatchTile ? n[b] - c : kBatchTile);
            }
    *ntiles = count;
    return PRG_OK;
}

int prg_cpd_batch_create(prg_cpd_batch** out, int device, void* hip_stream, int dim, int nb, const int64_t* source_offsets,
                         const int64_t* target_offsets, const double* sources, const double* targets) {
    PRG_REQUIRE(out && source_offsets && target_offsets && sources && targets, PRG_ERR_INVALID, "prg_cpd_batch_create: NULL argument");
    PRG_REQUIRE(dim == 2 || dim == 3, PRG_ERR_INVALID, "prg_cpd_batch_create: dim must be 2 or 3 (got %d)", dim);
    PRG_REQUIRE(nb > 0, PRG_ERR_INVALID, "prg_cpd_batch_create: need at least one problem");
    PRG_REQUIRE(source_offsets[0] == 0 && target_offsets[0] == 0, PRG_ERR_INVALID, "prg_cpd_batch_create: offset tables start at 0");
    std::vector<int64_t> m((size_t)nb), n((size_t)nb);
    for (int b = 0; b < nb; ++b) {
        m[(size_t)b] = source_offsets[b + 1] - source_offsets[b];
        n[(size_t)b] = target_offsets[b + 1] - target_offsets[b];
    }
    PRG_TRY(check_sizes("prg_cpd_batch_create", nb, m.data(), n.data()));
    int64_t nt = 0;
    PRG_TRY(prg_cpd_batch_tile_table(nb, m.data(), n.data(), nullptr, 0, &nt));
    PRG_REQUIRE(nt < (1ll << 31) - 1, PRG_ERR_INVALID, "prg_cpd_batch_create: %lld tiles do not fit one grid", (long long)nt);
    // host side of the layout: fp32 points (what the single plan uploads), the tile table and every problem's first tile
    const int64_t mtot = source_offsets[nb], ntot = target_offsets[nb];
    std::vector<float4> s4((size_t)mtot), t4((size_t)ntot);
    for (int64_t i = 0; i < mtot; ++i)
        s4[(size_t)i] = make_float4((float)sources[i * dim], (float)sources[i * dim + 1], dim > 2 ? (float)sources[i * dim + 2] : 0.f, 0.f);
    for (int64_t i = 0; i < ntot; ++i)
        t4[(size_t)i] = make_float4((float)targets[i * dim], (float)targets[i * dim + 1], dim > 2 ? (float)targets[i * dim + 2] : 0.f, 0.f);
    std::vector<int> t3((size_t)nt * 3);
    int64_t again = 0;
    (void)prg_cpd_batch_tile_table(nb, m.data(), n.data(), t3.data(), nt, &again);
    std::vector<int4> tiles((size_t)nt);
    std::vector<int> first((size_t)nb + 1, 0);
    for (int64_t i = 0; i < nt; ++i) {
        tiles[(size_t)i] = make_int4(t3[3 * i], t3[3 * i + 1], t3[3 * i + 2], 0);
        first[(size_t)t3[3 * i] + 1] = (int)i + 1;
    }
    // the handle comes AFTER the host vectors, which this function owns: on a failure of the set-up its buffers are freed - which
    // drains the stream and the uploads still queued from those vectors - before the vectors go
    return prg::create_handle(__func__, out, device, hip_stream, [&](prg_cpd_batch* h) -> int {
        h->dim = dim;
        h->B = nb;
        h->ntiles = (int)nt;
        h->Mtot = mtot;
        h->Ntot = ntot;
        auto put = [h](auto& buf, const auto* host, size_t count) -> int {
            PRG_HIP(buf.reset((int64_t)count));
            PRG_HIP(hipMemcpyAsync(buf.p, host, count * sizeof(*host), hipMemcpyHostToDevice, h->stream));
            return PRG_OK;
        };
        auto zeroed = [h](auto& buf, size_t count) -> int {
            PRG_HIP(buf.reset((int64_t)count));
            PRG_HIP(hipMemsetAsync(buf.p, 0, count * sizeof(*buf.p), h->stream));
            return PRG_OK;
        };
        PRG_TRY(put(h->src4, s4.data(), s4.size()));
        PRG_TRY(put(h->tgt4, t4.data(), t4.size()));
        PRG_TRY(put(h->soff, source_offsets, (size_t)nb + 1));
        PRG_TRY(put(h->toff, target_offsets, (size_t)nb + 1));
        PRG_TRY(put(h->tiles, tiles.data(), tiles.size()));
        PRG_TRY(put(h->tile_first, first.data(), first.size()));
        PRG_TRY(zeroed(h->params, (size_t)nb * PRG_NPARAMS));
        PRG_TRY(zeroed(h->part, (size_t)nt * kBatchComp));
        PRG_TRY(zeroed(h->init, (size_t)nb * 16));
        PRG_TRY(zeroed(h->wtol, (size_t)nb * 2));
        PRG_TRY(zeroed(h->flags, (size_t)nb * 2 + 1));
        PRG_HIP(h->pinned.ensure((int64_t)nb * 2 + 8));
        PRG_HIP(hipStreamSynchronize(h->stream));  // (the uploads read this call's own host vectors)
        return PRG_OK;
    });
}

int prg_cpd_batch_destroy(prg_cpd_batch* h) {
    return prg::destroy_handle(h);
}

int prg_cpd_batch_init(prg_cpd_batch* h, const double* init_params_host) {
    PRG_REQUIRE(h, PRG_ERR_INVALID, "prg_cpd_batch_init: NULL handle");
    PRG_ENTER(h->device);
    if (init_params_host)
        PRG_HIP(hipMemcpyAsync(h->init.p, init_params_host, (size_t)h->B * 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    k_batch_init<<<h->B, 256, 0, h->stream>>>(h->src4.p, h->tgt4.p, h->soff.p, h->toff.p, init_params_host ? h->init.p : nullptr, h->params.p,
                                              h->flags.p, h->B, h->dim);
    PRG_HIP(hipGetLastError());
    if (init_params_host) PRG_HIP(hipStreamSynchronize(h->stream));  // the caller may reuse its buffer
    h->initialised = true;
    return PRG_OK;
}

static int read_active(prg_cpd_batch* h, int* active) {
    int* slot = reinterpret_cast<int*>(h->pinned.p + (size_t)h->B * 2);
    PRG_HIP(hipMemcpyAsync(slot, h->flags.p + 2 * h->B, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PRG_HIP(hipStreamSynchronize(h->stream));
    *active = *slot;
    return PRG_OK;
}

int prg_cpd_batch_iterate(prg_cpd_batch* h, int kind, int update_scale, const double* w, const double* tol, int n_iter) {
    PRG_REQUIRE(h && w && tol, PRG_ERR_INVALID, "prg_cpd_batch_iterate: NULL argument");
    PRG_REQUIRE(h->initialised, PRG_ERR_STATE, "prg_cpd_batch_iterate: prg_cpd_batch_init has not run");
    PRG_REQUIRE(kind == PRG_TF_RIGID || kind == PRG_TF_AFFINE, PRG_ERR_INVALID,
                "prg_cpd_batch_iterate: kind must be PRG_TF_RIGID or PRG_TF_AFFINE");
    PRG_REQUIRE(n_iter >= 0, PRG_ERR_INVALID, "prg_cpd_batch_iterate: n_iter must be >= 0");
    bool may_stop = false;
    for (int b = 0; b < h->B; ++b) {
        PRG_REQUIRE(w[b] >= 0.0 && w[b] < 1.0, PRG_ERR_INVALID, "prg_cpd_batch_iterate: w[%d] = %g is outside [0, 1)", b, w[b]);
        may_stop = may_stop || !(tol[b] < 0.0);
    }
    PRG_ENTER(h->device);
    // w and tol are uploaded only when they differ from what the device holds: through the plan's pinned block, whose previous
    // copy has to be over before it is overwritten (a wait at the door, once per change - never between two iterations)
    std::vector<double> now(w, w + h->B);
    now.insert(now.end(), tol, tol + h->B);
    if (now != h->wtol_host) {
        PRG_HIP(hipStreamSynchronize(h->stream));
        memcpy(h->pinned.p, now.data(), now.size() * sizeof(double));
        PRG_HIP(hipMemcpyAsync(h->wtol.p, h->pinned.p, now.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->wtol_host.swap(now);
    }
    for (int it = 0; it < n_iter; ++it) {
        if (may_stop && it > 0 && it % kPoll == 0) {  // the one host round trip: every kPoll iterations, and only if a problem can stop
            int active = 0;
            PRG_TRY(read_active(h, &active));
            if (active == 0) break;
        }
        if (kind == PRG_TF_AFFINE)
            k_batch_sweep<true><<<h->ntiles, kBatchTile, 0, h->stream>>>(h->tiles.p, h->src4.p, h->tgt4.p, h->soff.p, h->toff.p, h->params.p,
                                                                        h->flags.p, h->wtol.p, h->part.p, h->dim);
        else
            k_batch_sweep<false><<<h->ntiles, kBatchTile, 0, h->stream>>>(h->tiles.p, h->src4.p, h->tgt4.p, h->soff.p, h->toff.p, h->params.p,
                                                                         h->flags.p, h->wtol.p, h->part.p, h->dim);
        k_batch_mstep<<<h->B, 64, 0, h->stream>>>(h->part.p, h->tile_first.p, h->params.p, h->flags.p, h->wtol.p + h->B, h->B, kind,
                                                  update_scale, h->dim);
    }
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int prg_cpd_batch_active(prg_cpd_batch* h, int* active) {
    PRG_REQUIRE(h && active, PRG_ERR_INVALID, "prg_cpd_batch_active: NULL argument");
    PRG_REQUIRE(h->initialised, PRG_ERR_STATE, "prg_cpd_batch_active: prg_cpd_batch_init has not run");
    PRG_ENTER(h->device);
    return read_active(h, active);
}

int prg_cpd_batch_get_params(prg_cpd_batch* h, double* params_host, int* n_iter_host) {
    PRG_REQUIRE(h && params_host, PRG_ERR_INVALID, "prg_cpd_batch_get_params: NULL argument");
    PRG_REQUIRE(h->initialised, PRG_ERR_STATE, "prg_cpd_batch_get_params: prg_cpd_batch_init has not run");
    PRG_ENTER(h->device);
    PRG_TRY(prg::copy_out(params_host, h->params, (int64_t)h->B * PRG_NPARAMS, h->stream));
    return prg::copy_out(n_iter_host, h->flags, h->B, h->stream, h->B);
}

}  // extern "C"
