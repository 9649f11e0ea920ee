// The geometry of the multi-level cell-grid search (the kernels are in grid_search.hip): which cells a
// shell of a level holds, which of them can matter, and what everything beyond a shell is farther than.  These few expressions
// are the correctness argument of the 1-NN walk, the k-NN walk and the radius count, so they exist once, as plain inline
// functions that the host compiles too (tests/host/grid_search_check.cpp walks them on the CPU against brute force).
//
// Unlike those of cell_grid.h, these expressions can contract into FMAs, and a restatement in plain IEEE arithmetic must take
// the same branches: every .hip file that includes this header starts with `#pragma clang fp contract(off)` before its
// includes, and a host build passes -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdlib.h>

#include "cell_grid.h"

namespace prg {

constexpr double kReach = 1.0 + 1.0e-12;  // the stop bound is a hair smaller than (s h)^2 + D^2: covers the rounding of d2
constexpr int kMaxLevels = 16;            // grids of growing cell edge: kLevelStep^(kMaxLevels - 1) = 2^kFloorBits
constexpr int kFloorBits = 30;            // no cell edge is below the largest extent / 2^kFloorBits
constexpr double kLevelStep = 4.0;        // edge of a level / edge of the level below
constexpr int kLevelShells = 2;           // shells 0 .. kLevelShells of a level are walked before the next level takes over
constexpr int kCountSpan = 4;  // the radius count walks the finest level on which the cube around r spans <= kCountSpan + 1 cells an axis

struct Levels {
    int count;
    CellGrid g[kMaxLevels];
    const double4* sp[kMaxLevels];  // the points in the cell order of the level, original index in .w
    const int2* cells[kMaxLevels];  // (begin, end) of every bucket
};

__host__ __device__ inline int lesser(int a, int b) { return a < b ? a : b; }
__host__ __device__ inline int greater(int a, int b) { return a > b ? a : b; }

// the query's cell, clamped into the grid: the centre of the shells
__host__ __device__ inline void centre_cell(const double (&q)[3], const CellGrid& g, int (&c)[3]) {
    for (int a = 0; a < 3; ++a) c[a] = lesser(cell_of(q[a], g.lo[a], g.edge), g.dim[a] - 1);
}

// The clip: the cells lo .. hi that can hold a point at most rho (a hair more) from q.  cell_of is monotone, so a point in a
// cell below lo[a] has y_a < q_a - rho and d2 > rho^2, and likewise above hi[a].
__host__ __device__ inline void clip_cells(const double (&q)[3], double rho, const CellGrid& g, int (&lo)[3], int (&hi)[3]) {
    for (int a = 0; a < 3; ++a) {
        const double wide = rho + (fabs(q[a]) + rho) * 0x1p-50;  // the rounding of q_a -+ rho
        lo[a] = lesser(cell_of(q[a] - wide, g.lo[a], g.edge), g.dim[a] - 1);
        hi[a] = lesser(cell_of(q[a] + wide, g.lo[a], g.edge), g.dim[a] - 1);
    }
}

// the last shell around c that meets the clip
__host__ __device__ inline int clip_shells(const int (&c)[3], const int (&lo)[3], const int (&hi)[3]) {
    int smax = 0;
    for (int a = 0; a < 3; ++a) smax = greater(smax, greater(c[a] - lo[a], hi[a] - c[a]));
    return smax;
}

// shell s around c: the cells at Chebyshev distance s
__host__ __device__ inline bool on_shell(int x, int y, int z, const int (&c)[3], int s) {
    const int dx = abs(x - c[0]), dy = abs(y - c[1]), dz = abs(z - c[2]);
    return greater(dx, greater(dy, dz)) == s;
}

// squared distance of the query to the cloud's box, shrunk by a hair
__host__ __device__ inline double box_distance2(const double (&q)[3], const CellGrid& g) {
    double box2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        const double lo = g.lo[a], hi = g.hi[a];
        const double out = q[a] < lo ? lo - q[a] : (q[a] > hi ? q[a] - hi : 0.0);
        box2 += out * out;
    }
    return box2 / kReach;
}

// After shell s, what is not visited yet lies in cells at Chebyshev distance > s of the clamped cell: its d2 exceeds this.
__host__ __device__ inline double shell_bound(int s, const CellGrid& g, double box2) {
    const double reach = fmax((double)s - g.slack, 0.0) * g.edge / kReach;
    return reach * reach + box2;
}

// The radius walk: every point that can lie within r of q goes to visit(p) exactly once (p: the point, its original index in
// .w).  It runs on one level, the finest on which the cells that can hold such a point span at most kCountSpan + 1 an axis
// (the last level otherwise).  Every point is in one cell of a level and every cell of the cube is visited once; on a hashed
// level a bucket may hold points of other cells, which are left to their own cell.  The visitor decides d2 <= r r itself.  The
// level loop is uniform.  The radius count and the DBSCAN link of the ICP plan are this walk with two visitors.
template <class Visit>
__host__ __device__ inline void radius_walk(const Levels& lv, const double (&q)[3], double r, Visit& visit) {
    const double rho = r * kReach;
    bool done = false;
    for (int v = 0; v < lv.count; ++v) {
        if (done) continue;
        const CellGrid& g = lv.g[v];
        int lo[3], hi[3];
        clip_cells(q, rho, g, lo, hi);
        const int span = greater(hi[0] - lo[0], greater(hi[1] - lo[1], hi[2] - lo[2]));
        if (span > kCountSpan && v + 1 < lv.count) continue;
        done = true;
        const double4* __restrict__ sp = lv.sp[v];
        const int2* __restrict__ cells = lv.cells[v];
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const int2 be = cells[cell_key(x, y, z, g)];
                    for (int t = be.x; t < be.y; ++t) {
                        const double4 p = sp[t];
                        if (!g.dense && (cell_of(p.x, g.lo[0], g.edge) != x || cell_of(p.y, g.lo[1], g.edge) != y ||
                                         cell_of(p.z, g.lo[2], g.edge) != z))
                            continue;
                        visit(p);
                    }
                }
    }
}

}  // namespace prg
