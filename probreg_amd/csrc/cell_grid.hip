// The builder of the cell grid of cell_grid.h: key per point, stable sort, bucket bounds and gather - and the host loop that
// brings a cloud in for it.  The cell of a point is a decision value: no contraction into FMAs (as in the grid's two users).
#pragma clang fp contract(off)
#include "cell_grid.h"

#include <algorithm>
#include <cmath>

#include "lattice_sort.h"
#include "prg_common.h"

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_cell_keys(const double4* __restrict__ pts, int64_t n, prg::CellGrid g,
                                                      unsigned* __restrict__ keys, int* __restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const double4 p = pts[t];
    keys[t] = prg::cell_key(prg::cell_of(p.x, g.lo[0], g.edge), prg::cell_of(p.y, g.lo[1], g.edge),
                            prg::cell_of(p.z, g.lo[2], g.edge), g);
    vals[t] = (int)t;
}

// points (index in .w) in cell order, and (begin, end) of every bucket (zeroed before): the first and the last thread of a
// run of equal keys write them, whichever workgroups they are in
__global__ __launch_bounds__(kBlock) void k_cell_bounds(const double4* __restrict__ pts, const unsigned* __restrict__ skeys,
                                                        const int* __restrict__ order, int64_t n, double4* __restrict__ sp,
                                                        int2* __restrict__ cells) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const int i = order[t];
    double4 p = pts[i];
    p.w = (double)i;
    sp[t] = p;
    const unsigned key = skeys[t];
    if (t == 0 || skeys[t - 1] != key) cells[key].x = (int)t;
    if (t == n - 1 || skeys[t + 1] != key) cells[key].y = (int)(t + 1);
}

}  // namespace

namespace prg {

int CellGridScratch::size(int64_t n, unsigned bits) {
    PRG_HIP(keys.reset(2 * n));
    PRG_HIP(vals.reset(2 * n));
    tmp_bytes = 0;
    PRG_TRY(sort_pairs_u32(nullptr, &tmp_bytes, keys.p, keys.p + n, vals.p, vals.p + n, (unsigned)n, bits, nullptr));
    PRG_HIP(tmp.reset((int64_t)tmp_bytes + 256));
    return PRG_OK;
}

int build_cell_grid(const CellGrid& g, unsigned bits, const double4* pts, int64_t n, CellGridScratch& s, double4* sp_out,
                    int2* cells_out, hipStream_t stream) {
    const unsigned nb = (unsigned)ceil_div(n, kBlock);
    unsigned* const keys = s.keys.p;
    int* const vals = s.vals.p;
    k_cell_keys<<<nb, kBlock, 0, stream>>>(pts, n, g, keys, vals);
    PRG_HIP(hipGetLastError());
    PRG_TRY(sort_pairs_u32(s.tmp.p, &s.tmp_bytes, keys, keys + n, vals, vals + n, (unsigned)n, bits, stream));
    PRG_HIP(hipMemsetAsync(cells_out, 0, (size_t)cell_entries(g) * sizeof(int2), stream));
    k_cell_bounds<<<nb, kBlock, 0, stream>>>(pts, keys + n, vals + n, n, sp_out, cells_out);
    PRG_HIP(hipGetLastError());
    return PRG_OK;
}

int load_cloud3(const double* points_hd, int64_t n, int dim, const char* not_finite, std::vector<double>& raw,
                std::vector<double>& pad, double* lo, double* hi) {
    raw.resize((size_t)n * dim);
    pad.resize((size_t)n * 4, 0.0);  // only columns 0 .. 2 are written below: a pad that is used again keeps its zeros
    PRG_HIP(hipMemcpy(raw.data(), points_hd, raw.size() * sizeof(double), hipMemcpyDefault));
    double b[2][3];  // the box in locals: through lo and hi, which may alias pad, every update would go through memory
    for (int a = 0; a < 3; ++a) b[0][a] = b[1][a] = a < dim ? raw[a] : 0.0;
    for (int64_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) {
            const double v = a < dim ? raw[(size_t)i * dim + a] : 0.0;
            PRG_REQUIRE(!not_finite || std::isfinite(v), PRG_ERR_INVALID, "%s", not_finite);
            pad[(size_t)i * 4 + a] = v;
            b[0][a] = std::min(b[0][a], v);
            b[1][a] = std::max(b[1][a], v);
        }
    for (int a = 0; a < 3 && lo; ++a) lo[a] = b[0][a], hi[a] = b[1][a];
    return PRG_OK;
}

}  // namespace prg
