// The ICP plan and what its four translation units share: icp.hip (lifecycle, clouds, sums, step, loop), grid_search.hip (the
// levels and the searches on them), icp_outlier.hip (the two filters on the lists and counts) and icp_cluster.hip (DBSCAN on the
// counts and the radius walk).  Only host functions cross a file; each kernel is launched from the file that defines it.
#pragma once
#include "dev_buf.h"
#include "grid_search.h"
#include "prg_common.h"

namespace prg {
namespace icp {

constexpr int kBlock = 256;
constexpr int kRun = 64;    // source points per run of the ordered sums (part of the definition)
constexpr int kSlots = 32;  // sums per run: 8 / 9 (point-to-point, two passes), 29 (point-to-plane), 30 (generalized)

// state (doubles)
constexpr int kStPose = 0, kStCentre = 12, kStStop = 18, kStCount = 19, kStSum = 20, kStFitness = 21, kStRmse = 22,
              kStIter = 23, kStConverged = 24, kStStatus = 25, kStEvals = 26, kStSumsA = 32, kStSumsB = 64, kStLen = 96;

// q_a = ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) + t_a
__device__ __forceinline__ void moved(const double (&m)[12], const double* __restrict__ p, double (&q)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = ((m[3 * a] * p[0] + m[3 * a + 1] * p[1]) + m[3 * a + 2] * p[2]) + m[9 + a];
}

// source point m under the pose in the state: the query of every search
__device__ __forceinline__ void moved_query(const double* __restrict__ state, const double* __restrict__ src, int64_t m,
                                            double (&q)[3]) {
    double pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = state[kStPose + k];
    moved(pose, src + m * 3, q);
}

}  // namespace icp
}  // namespace prg

struct prg_icp {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t N = 0, M = 0;
    bool have_normals = false, have_order = false, have_matches = false;
    int have_knn = 0;                          // k of the lists in knn_*, 0: none
    bool have_counts = false;
    int have_outlier = 0;                      // 0 none, 1 statistical (score, stat, keep), 2 radius (counts, keep)
    bool have_dbscan = false;                  // db_* hold a clustering (of the counts in `counts`)
    int db_clusters = -1;                      // its number of clusters once it has been read back, -1: not yet
    bool have_cov[2] = {false, false};         // source, target
    prg::Levels lv;
    prg::DevBuf<double4> tp, tn;               // target points and normals, padded to four doubles
    prg::DevBuf<double4> sp[prg::kMaxLevels];  // per level: the points in cell order, original index in .w
    prg::DevBuf<int2> cells[prg::kMaxLevels];  // per level, table entries: (begin, end)
    prg::DevBuf<double> src;                   // [M][3]
    prg::DevBuf<double> cov[2];                // [M][6] of the source, [N][6] of the target
    prg::DevBuf<unsigned> qkeys;               // 2 M: unsorted, sorted
    prg::DevBuf<int> qvals;                    // 2 M: iota, order
    prg::DevBuf<char> sort_tmp;
    prg::DevBuf<int> idx;                      // [M]
    prg::DevBuf<double> d2;                    // [M]
    prg::DevBuf<double> part;                  // [runs][kSlots]
    prg::DevBuf<double> state;                 // [kStLen]
    prg::DevBuf<int> knn_idx;                  // [M][k]
    prg::DevBuf<double> knn_d2;                // [M][k]
    prg::DevBuf<int> knn_cnt;                  // [M]
    prg::DevBuf<int> counts;                   // [M]: the radius count
    prg::DevBuf<double> score;                 // [M]: the mean neighbour distance
    prg::DevBuf<double> stat;                  // mu, s, thr
    prg::DevBuf<unsigned char> keep;           // [M]
    prg::DevBuf<unsigned char> db_core;        // [M]: 1 core, 0 not
    prg::DevBuf<int> db_parent;                // [M]: the union-find over the core points, -1 for the others
    prg::DevBuf<int> db_near;                  // [M]: the nearest core neighbour of a point that is not core, -1: none
    prg::DevBuf<int> db_id;                    // [M]: the cluster number, at the roots only
    prg::DevBuf<int> db_labels;                // [M]
    prg::DevBuf<int> db_sizes;                 // [M]: the first db_clusters are used
    prg::DevBuf<int> db_tiles;                 // [2 tiles + 1]: roots per tile, their scan, the number of clusters
};

namespace prg {
namespace icp {

// icp.hip
int require_ready(prg_icp* h, const char* who, bool matches);  // a target and a source; `matches`: and a search on them
void drop_lists(prg_icp* h);  // lists, counts and filter results belong to the clouds and the pose they were made with

// grid_search.hip
// The levels of the target in h->tp (n points, the box lo .. hi; raw: its rows on the host) from cell_edge, or from the cloud
// when it is 0.  Synchronises the stream.
int build_levels(prg_icp* h, const std::vector<double>& raw, int64_t n, const double* lo, const double* hi, double cell_edge);
int ensure_order(prg_icp* h);               // the queries in Morton order of their position under the current pose
void enqueue_search(prg_icp* h, double r);  // the matches of every moved source point into idx, d2
int run_knn(prg_icp* h, const char* who, int k, double r);     // the k-best lists into knn_*; the buffers grow to M k
int run_radius_count(prg_icp* h, const char* who, double r);   // the radius counts into counts

}  // namespace icp
}  // namespace prg
