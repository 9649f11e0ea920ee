// Host check of probreg_amd/csrc/grid_search.h (tests/test_grid_search_host.py builds this with the host compiler under
// AddressSanitizer / UBSan with -ffp-contract=off and runs it; no HIP runtime, no GPU).  A plain CPU shell loop drives the
// header's centre cell, clip, shell predicate, box distance and bound the way walk_level of grid_search.hip does, over small
// clouds binned on the CPU with cell_grid.h, and compares with brute force:
//   - across the shells of one level every cell of the clipped cube is met exactly once;
//   - a finished walk holds exactly the k smallest (d2, index) of the whole cloud (among d2 <= r r), k = 1, 8, 64, and the
//     unfiltered single best of the 1-NN search - so a stop by the bound left nothing strictly better unvisited;
//   - the clip never excludes a point with d2 <= rho rho;
//   - the clipped cube of the level the kCountSpan rule picks counts every point with d2 <= r r, once.
// Grids: dense and hashed, two, three and four levels from a hand-given edge.  Queries: inside the cloud, on the faces and
// corners of its box, on cloud points, 10^6 extents away, and at coordinates near 2^52 edge, where q -+ rho rounds by about a
// cell and the 0x1p-50 widening of the clip matters.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../probreg_amd/csrc/grid_search.h"

using namespace prg;

static int g_failed = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                      \
        }                                                                    \
    } while (0)

typedef std::pair<double, int> Key;  // (d2, index): std::pair orders them as the search does

struct Rng {
    uint64_t s;
    double next() {  // [0, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * 0x1p-53;
    }
};

struct Level {
    CellGrid g;
    std::vector<std::vector<int> > bucket;
};

struct Cloud {
    std::vector<double> p;  // [n][3]
    int n;
    double lo[3], hi[3];
    std::vector<Level> lv;
};

static double dist2(const Cloud& c, int i, const double (&q)[3]) {
    const double dx = c.p[3 * i] - q[0], dy = c.p[3 * i + 1] - q[1], dz = c.p[3 * i + 2] - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the box, then the levels as prg_icp_set_target makes them from a given edge
static void finish_cloud(Cloud& c, double edge0) {
    c.n = (int)(c.p.size() / 3);
    for (int a = 0; a < 3; ++a) c.lo[a] = c.hi[a] = c.p[a];
    for (int i = 0; i < c.n; ++i)
        for (int a = 0; a < 3; ++a) {
            c.lo[a] = std::min(c.lo[a], c.p[3 * i + a]);
            c.hi[a] = std::max(c.hi[a], c.p[3 * i + a]);
        }
    const unsigned bits = cell_table_bits(c.n);
    double edge = edge0;
    for (int k = 0; k < kMaxLevels; ++k, edge *= kLevelStep) {
        Level l;
        l.g = make_cell_grid(c.lo, c.hi, edge, bits);
        l.bucket.resize((size_t)cell_entries(l.g));
        for (int i = 0; i < c.n; ++i)
            l.bucket[cell_key(cell_of(c.p[3 * i], c.lo[0], edge), cell_of(c.p[3 * i + 1], c.lo[1], edge),
                              cell_of(c.p[3 * i + 2], c.lo[2], edge), l.g)]
                .push_back(i);
        c.lv.push_back(l);
        if (std::max(l.g.dim[0], std::max(l.g.dim[1], l.g.dim[2])) <= 2) break;
    }
    const CellGrid& last = c.lv.back().g;
    CHECK(std::max(last.dim[0], std::max(last.dim[1], last.dim[2])) <= 2);
}

// every cell of the cube lo .. hi lies on exactly one of the shells 0 .. clip_shells around c
static void check_shells(const CellGrid& g, const double (&q)[3], double rho) {
    int c[3], lo[3], hi[3];
    centre_cell(q, g, c);
    clip_cells(q, rho, g, lo, hi);
    const int smax = clip_shells(c, lo, hi);
    for (int a = 0; a < 3; ++a) CHECK(0 <= lo[a] && lo[a] <= c[a] && c[a] <= hi[a] && hi[a] < g.dim[a]);
    const int nx = hi[0] - lo[0] + 1, ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
    if ((double)(smax + 1) * nx * ny * nz > 3.0e4) return;  // the loop below costs that much; the smaller grids cover whole boxes
    std::vector<int> met((size_t)nx * ny * nz, 0);
    for (int s = 0; s <= smax; ++s)
        for (int z = std::max(c[2] - s, lo[2]); z <= std::min(c[2] + s, hi[2]); ++z)
            for (int y = std::max(c[1] - s, lo[1]); y <= std::min(c[1] + s, hi[1]); ++y)
                for (int x = std::max(c[0] - s, lo[0]); x <= std::min(c[0] + s, hi[0]); ++x)
                    if (on_shell(x, y, z, c, s)) ++met[((size_t)(z - lo[2]) * ny + (y - lo[1])) * nx + (x - lo[0])];
    bool once = true;
    for (size_t i = 0; i < met.size(); ++i) once = once && met[i] == 1;
    CHECK(once);
}

// no point with d2 <= rho rho lies in a cell outside the clip, on any level
static void check_clip(const Cloud& c, const double (&q)[3], double rho) {
    for (size_t v = 0; v < c.lv.size(); ++v) {
        const CellGrid& g = c.lv[v].g;
        int lo[3], hi[3];
        clip_cells(q, rho, g, lo, hi);
        bool inside = true;
        for (int i = 0; i < c.n; ++i) {
            if (!(dist2(c, i, q) <= rho * rho)) continue;
            for (int a = 0; a < 3; ++a) {
                const int cell = cell_of(c.p[3 * i + a], g.lo[a], g.edge);
                inside = inside && lo[a] <= cell && cell <= hi[a];
            }
        }
        CHECK(inside);
    }
}

static int g_by_bound = 0, g_by_clip = 0, g_by_radius = 0, g_handed_over = 0;

// the walk of grid_search.hip: the k best among d2 <= r r (`filter`), or the best of all that is visited (the 1-NN list)
static std::vector<Key> walk(const Cloud& c, const double (&q)[3], int k, double r, bool filter) {
    const double r2 = r * r, box2 = box_distance2(q, c.lv[0].g);
    double rho = r * kReach;
    std::vector<Key> list;
    bool done = false;
    for (size_t v = 0; v < c.lv.size() && !done; ++v) {
        const Level& l = c.lv[v];
        const int shells = v + 1 < c.lv.size() ? kLevelShells : 0x7fffffff;
        if (v > 0) ++g_handed_over;
        int ctr[3], lo[3], hi[3];
        centre_cell(q, l.g, ctr);
        for (int s = 0;; ++s) {
            clip_cells(q, rho, l.g, lo, hi);
            if (s > clip_shells(ctr, lo, hi)) {
                ++g_by_clip;
                done = true;
                break;
            }
            if (s > shells) break;
            for (int z = std::max(ctr[2] - s, lo[2]); z <= std::min(ctr[2] + s, hi[2]); ++z)
                for (int y = std::max(ctr[1] - s, lo[1]); y <= std::min(ctr[1] + s, hi[1]); ++y)
                    for (int x = std::max(ctr[0] - s, lo[0]); x <= std::min(ctr[0] + s, hi[0]); ++x) {
                        if (!on_shell(x, y, z, ctr, s)) continue;
                        const std::vector<int>& b = l.bucket[cell_key(x, y, z, l.g)];
                        for (size_t t = 0; t < b.size(); ++t) {
                            const Key cand(dist2(c, b[t], q), b[t]);
                            if (filter && !(cand.first <= r2)) continue;
                            const std::vector<Key>::iterator at = std::lower_bound(list.begin(), list.end(), cand);
                            if ((at != list.end() && *at == cand) || at - list.begin() >= k) continue;  // a second visit; too far
                            list.insert(at, cand);
                            if ((int)list.size() > k) list.pop_back();
                        }
                    }
            const double bound = shell_bound(s, l.g, box2);
            const bool full = (int)list.size() == k;
            if ((full && list.back().first < bound) || bound > r2) {
                ++(full && list.back().first < bound ? g_by_bound : g_by_radius);
                done = true;
                break;
            }
            if (full) rho = fmin(rho, sqrt(list.back().first) * kReach);
        }
    }
    CHECK(done);  // the last level ends every walk
    return list;
}

// c(q) on the level of the kCountSpan rule, as k_icp_radius_count walks it
static int count_within(const Cloud& c, const double (&q)[3], double r) {
    const double rho = r * kReach, r2 = r * r;
    for (size_t v = 0; v < c.lv.size(); ++v) {
        const Level& l = c.lv[v];
        int lo[3], hi[3];
        clip_cells(q, rho, l.g, lo, hi);
        const int span = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
        if (span > kCountSpan && v + 1 < c.lv.size()) continue;
        int count = 0;
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y)
                for (int x = lo[0]; x <= hi[0]; ++x) {
                    const std::vector<int>& b = l.bucket[cell_key(x, y, z, l.g)];
                    for (size_t t = 0; t < b.size(); ++t) {
                        const double* p = &c.p[3 * b[t]];
                        if (!l.g.dense && (cell_of(p[0], l.g.lo[0], l.g.edge) != x || cell_of(p[1], l.g.lo[1], l.g.edge) != y ||
                                           cell_of(p[2], l.g.lo[2], l.g.edge) != z))
                            continue;  // a point of another cell in a hashed bucket: left to its own cell
                        count += dist2(c, b[t], q) <= r2 ? 1 : 0;
                    }
                }
        return count;
    }
    return -1;
}

static void check_query(const Cloud& c, const double (&q)[3], Rng& rng) {
    std::vector<Key> all((size_t)c.n);
    for (int i = 0; i < c.n; ++i) all[(size_t)i] = Key(dist2(c, i, q), i);
    std::sort(all.begin(), all.end());
    const double ext = std::max(c.hi[0] - c.lo[0], std::max(c.hi[1] - c.lo[1], c.hi[2] - c.lo[2]));
    const double reach = sqrt(all[(size_t)(rng.next() * c.n)].first);  // exactly up to some point of the cloud
    const double radii[5] = {INFINITY, 0.04 * ext, 0.6 * ext, reach, reach * (1.0 - 0x1p-30)};
    for (int ri = 0; ri < 5; ++ri) {
        const double r = radii[ri], r2 = r * r;
        if (!(r > 0.0)) continue;
        const size_t within = (size_t)(std::upper_bound(all.begin(), all.end(), Key(r2, 0x7fffffff)) - all.begin());
        // the 1-NN search: unfiltered, the kernel drops a best beyond r at the end
        const std::vector<Key> best = walk(c, q, 1, r, false);
        if (within > 0) CHECK(best.size() == 1 && best[0] == all[0]);
        else CHECK(best.empty() || best[0].first > r2);
        const int ks[3] = {1, 8, 64};
        for (int ki = 0; ki < 3; ++ki) {
            const std::vector<Key> got = walk(c, q, ks[ki], r, true);
            const size_t want = std::min(within, (size_t)ks[ki]);
            CHECK(got.size() == want && std::equal(got.begin(), got.end(), all.begin()));
        }
        check_clip(c, q, r * kReach);
        check_clip(c, q, r);
        for (size_t v = 0; v < c.lv.size(); ++v) check_shells(c.lv[v].g, q, r * kReach);
        if (r < INFINITY) CHECK(count_within(c, q, r) == (int)within);
    }
}

static void check_cloud(Cloud& c, double edge0, size_t levels, bool dense0, uint64_t seed) {
    finish_cloud(c, edge0);
    CHECK(c.lv.size() == levels && (c.lv[0].g.dense != 0) == dense0);
    Rng rng = {seed};
    const double ext = std::max(c.hi[0] - c.lo[0], std::max(c.hi[1] - c.lo[1], c.hi[2] - c.lo[2]));
    double mid[3], in[3];
    for (int a = 0; a < 3; ++a) mid[a] = 0.5 * (c.lo[a] + c.hi[a]);
    for (int t = 0; t < 8; ++t) {  // inside the box
        double q[3];
        for (int a = 0; a < 3; ++a) q[a] = c.lo[a] + rng.next() * (c.hi[a] - c.lo[a]);
        check_query(c, q, rng);
    }
    for (int t = 0; t < 3; ++t) {  // on points of the cloud
        const int i = (int)(rng.next() * c.n);
        const double q[3] = {c.p[3 * i], c.p[3 * i + 1], c.p[3 * i + 2]};
        check_query(c, q, rng);
    }
    for (int f = 0; f < 6; ++f) {  // on the six faces
        for (int a = 0; a < 3; ++a) in[a] = c.lo[a] + rng.next() * (c.hi[a] - c.lo[a]);
        in[f / 2] = f % 2 ? c.hi[f / 2] : c.lo[f / 2];
        const double q[3] = {in[0], in[1], in[2]};
        check_query(c, q, rng);
    }
    for (int t = 0; t < 3; ++t) {  // corners
        const double q[3] = {t == 0 ? c.lo[0] : c.hi[0], t == 1 ? c.hi[1] : c.lo[1], t == 2 ? c.lo[2] : c.hi[2]};
        check_query(c, q, rng);
    }
    const double far[2] = {1.0e6 * ext, ldexp(edge0, 52)};  // 10^6 extents away; where a coordinate resolves about one cell
    for (int w = 0; w < 2; ++w)
        for (int t = 0; t < 5; ++t) {  // along +x, -y, +z, a diagonal, and just off an axis through the cloud
            double q[3] = {mid[0], mid[1], mid[2]};
            if (t == 0 || t == 3) q[0] += far[w];
            if (t == 1 || t == 3) q[1] -= far[w];
            if (t == 2 || t == 3) q[2] += far[w];
            if (t == 4) {
                q[0] = c.lo[0] + rng.next() * (c.hi[0] - c.lo[0]);
                q[1] -= far[w];
                q[2] = c.hi[2];
            }
            check_query(c, q, rng);
        }
}

int main() {
    Rng rng = {12345};
    {  // 2000 points in a unit box, 11^3 cells: dense, three levels
        Cloud c;
        const double at[3] = {-0.3, 2.0, 5.0};
        for (int i = 0; i < 3 * 2000; ++i) c.p.push_back(at[i % 3] + rng.next());
        check_cloud(c, 0.1, 3, true, 1);
    }
    {  // 200 points, 21^3 cells against a table of 2^10: hashed, three levels
        Cloud c;
        for (int i = 0; i < 3 * 200; ++i) c.p.push_back(rng.next() - 0.5);
        check_cloud(c, 0.05, 3, false, 2);
    }
    {  // 500 points, 4^3 cells: dense, two levels
        Cloud c;
        for (int i = 0; i < 3 * 500; ++i) c.p.push_back(3.0 * rng.next());
        check_cloud(c, 0.9, 2, true, 3);
    }
    {  // two clusters ten apart and repeated points: 41^3 cells, nearly all empty: hashed, four levels
        Cloud c;
        for (int i = 0; i < 1000; ++i) {
            const double shift = i % 2 ? 10.0 : 0.0;
            for (int a = 0; a < 3; ++a) c.p.push_back(shift + 0.2 * rng.next());
        }
        for (int i = 0; i < 3 * 40; ++i) c.p.push_back(c.p[(size_t)i]);
        check_cloud(c, 0.25, 4, false, 4);
    }
    {  // coordinates of 2^44 with an extent of 4096: the points themselves resolve 2^-8
        Cloud c;
        for (int i = 0; i < 3 * 1200; ++i) c.p.push_back(0x1p44 + 4096.0 * rng.next());
        check_cloud(c, 300.0, 3, true, 5);
    }
    // every way a walk can end was taken, and coarser levels took over
    CHECK(g_by_bound > 100 && g_by_clip > 100 && g_by_radius > 100 && g_handed_over > 100);
    if (g_failed) {
        fprintf(stderr, "grid_search_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("grid_search_check ok (%d walks ended by the bound, %d by the clip, %d by the radius; %d level hand-overs)\n",
           g_by_bound, g_by_clip, g_by_radius, g_handed_over);
    return 0;
}
