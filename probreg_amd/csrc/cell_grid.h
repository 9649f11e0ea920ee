// The library's one cell grid (DESIGN.md section 3.9 is its definition), which the FPFH search (fpfh.hip) and the ICP search
// (grid_search.hip) bin a cloud with: clamped cell coordinates, row-major keys while the box fits the table and hashed ones otherwise,
// points sorted stably by key, one (begin, end) per bucket.  The descriptor part (down to cell_entries) is host-compilable
// against the HIP runtime API alone, as dev_buf.h is (tests/host/cell_grid_check.cpp); the builder is cell_grid.hip.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "dev_buf.h"

namespace prg {

constexpr double kCellMax = 1073741823.0;  // cell coordinates are clamped to [0, 2^30)
constexpr unsigned kMinTableBits = 10, kMaxTableBits = 26;

struct CellGrid {
    double lo[3], hi[3];  // the cloud's box
    double edge;
    double slack;         // cells: what the rounding of (x - lo) / edge can move a cell difference by
    int dim[3];
    unsigned mask;        // table - 1
    int dense;
};

// Monotone in x and clamped: neighbours within one edge stay within one cell whatever the magnitudes, and a difference of
// clamped cells never exceeds the difference of the unclamped ones.  A subtraction, a division, a floor and two selects:
// nothing here can contract into an FMA, so the including file's fp-contract setting does not matter.
__host__ __device__ inline int cell_of(double x, double lo, double edge) {
    double c = floor((x - lo) / edge);
    c = c > 0.0 ? c : 0.0;  // (also NaN -> 0)
    c = c < kCellMax ? c : kCellMax;
    return (int)c;
}

__host__ __device__ inline unsigned cell_key(int cx, int cy, int cz, const CellGrid& g) {
    if (g.dense) return ((unsigned)cz * (unsigned)g.dim[1] + (unsigned)cy) * (unsigned)g.dim[0] + (unsigned)cx;
    // Teschner et al. 2003, "Optimized spatial hashing for collision detection of deformable objects"
    const uint64_t h = ((uint64_t)cx * 73856093ull) ^ ((uint64_t)cy * 19349663ull) ^ ((uint64_t)cz * 83492791ull);
    return (unsigned)(h ^ (h >> 29)) & g.mask;
}

// log2 of the table size of a cloud of n points
inline unsigned cell_table_bits(int64_t n) {
    unsigned bits = kMinTableBits;
    while (bits < kMaxTableBits && ((int64_t)1 << bits) < 2 * n) ++bits;
    return bits;
}

inline CellGrid make_cell_grid(const double* lo, const double* hi, double edge, unsigned bits) {
    CellGrid g;
    g.edge = edge;
    g.mask = (1u << bits) - 1u;
    double cells = 1.0;
    int dim_max = 1;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo[a];
        g.hi[a] = hi[a];
        g.dim[a] = cell_of(hi[a], lo[a], edge) + 1;
        cells *= (double)g.dim[a];
        dim_max = g.dim[a] > dim_max ? g.dim[a] : dim_max;
    }
    g.dense = cells <= (double)g.mask + 1.0 ? 1 : 0;
    g.slack = ldexp((double)dim_max + 1.0, -48);
    return g;
}

// buckets: a dense grid needs one per cell, no more
inline int64_t cell_entries(const CellGrid& g) {
    return g.dense ? (int64_t)g.dim[0] * g.dim[1] * g.dim[2] : (int64_t)g.mask + 1;
}

// What a build needs besides its outputs; the caller drops it after the synchronisation that follows its builds.
struct CellGridScratch {
    DevBuf<unsigned> keys;  // 2 n: unsorted, sorted
    DevBuf<int> vals;       // 2 n: iota, order
    DevBuf<char> tmp;       // of the sort
    size_t tmp_bytes = 0;
    int size(int64_t n, unsigned bits);
};

// Enqueues keys -> stable sort -> zeroed buckets -> bounds and gather for the n points `pts`: sp_out [n] gets the points in
// cell order with the original index in .w, cells_out [cell_entries(g)] the (begin, end) of every bucket.  No synchronisation.
int build_cell_grid(const CellGrid& g, unsigned bits, const double4* pts, int64_t n, CellGridScratch& scratch, double4* sp_out,
                    int2* cells_out, hipStream_t stream);

// Copies n rows of `dim` (2 or 3) doubles in (host or device memory); PRG_ERR_INVALID with the message `not_finite` if one
// is not finite (NULL: not checked).  raw [n][dim]: the rows; pad [n][4]: (x, y, z or 0, 0) per row (pad comes in empty or from
// an earlier call); lo, hi: the box, or NULL.  The library's one loader of a cloud into the padded layout.
int load_cloud3(const double* points_hd, int64_t n, int dim, const char* not_finite, std::vector<double>& raw,
                std::vector<double>& pad, double* lo, double* hi);

}  // namespace prg
