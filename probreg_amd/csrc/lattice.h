// The permutohedral lattice (lattice.hip) as its two users see it: the stand-alone filter (prg_ph_*, in lattice.hip itself) and
// the FilterReg plan (filterreg.hip), which builds a lattice over its own clouds every E-step and slices inside its M-step.
#pragma once
#include "dev_buf.h"
#include "prg_common.h"

namespace prg {

// Feature producer of the FilterReg plan (filterreg.py:84-85 fused into the embedding): point i < m is the transformed
// source z = R y + t (kept as fp64 for the M-step), point i >= m a target point; both are divided by sigma in fp64
// before the float32 cast, exactly the reference's `t_source / sigma`, `target / sigma` followed by pybind's cast.
struct FrFeat {
    const double* src;
    const double* tgt;
    const double* state;  // [0..8] rot, [9..11] t, [12] sigma2
    double* ts;           // [m][3] transformed source (written by whoever embeds a source point)
    int64_t m;
    int dim;
};

// what the resolve kernel publishes to the host (see k_resolve)
struct LatticeMail { int size, overflow, side_size, side_overflow; unsigned seq; unsigned pad[3]; };

// Every buffer owns its memory (dev_buf.h): deleting the handle (destroy_handle, plan_base.h: on its device, after the stream
// has drained) releases everything.
struct Lattice {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0;   // embedded points
    int d = 0;       // feature dimension the build buffers below were created for (0: none)
    int with_blur = 1;
    int size = 0;    // number of lattice vertices (host copy)
    const float* pend_vals = nullptr;   // lat_filter(defer_slice): the final value plane, waiting to be sliced
    float pend_alpha = 0.f;
    // device
    DevBuf<float> feat;                 // [n][d]
    // the five build buffers are created together, for exactly the n and d of a build that does not fit the present ones
    DevBuf<unsigned long long> tkeys;   // hash table [tkeys.cap], a power of two
    DevBuf<int> slot_id;                // [tkeys.cap] dense id of an occupied slot
    DevBuf<int> pslot;                  // [n][d+1] slot, later overwritten by dense id (= offset_)
    DevBuf<float> bary;                 // [n][d+1]
    DevBuf<unsigned long long> dkeys;   // [n*(d+1)] dense keys
    DevBuf<int> nb;                     // [2][d+1][size] blur neighbours (dense id or -1)
    DevBuf<int> count;                  // device counters: [0] vertices, [1] table overflow flag
    int64_t cap_used = 0;               // slots of the table in use for the current build (power of two <= tkeys.cap)
    // d <= 3: a table entry is (generation << 48) | packed key; an entry of another generation counts as empty, so a
    // build starts by taking the next generation instead of clearing the table (gen 0 = freshly zeroed memory)
    unsigned gen = 0, gen2 = 0;
    int prev_size[2] = {0, 0};          // last lattice size without / with blur: sizes the next hash table
    int attempts = 0;                   // table attempts of the last d <= 3 build (2: it was retried at full capacity)
    HostBuf<double> pinned;             // 64 doubles of pinned host memory: small device->host read-backs (a copy
                                        // into pageable memory costs ~100 us of staging, this one a few us)
    bool built = false;                 // false after a decision-only build that stopped early (lat_build)
    DevBuf<float> vals;                 // [2][(size+1)][C] ping-pong value buffers
    DevBuf<float> io;                   // staging for values / outputs
    const FrFeat* prod = nullptr;       // non-null: features come from the FilterReg plan's clouds, not from `feat`
    // side table of the speculative with_blur decision (fr_build): a 1/16 subset of the points, hashed with the
    // blur scaling while the non-blur lattice is built in the main table; side[0] vertices, side[1] overflow
    DevBuf<unsigned long long> tkeys2;
    DevBuf<int> count2;
    bool side_pending = false;
    bool side_fuse = false;            // the side stage is prepared and rides in the next build's first embedding launch
    int side_size = 0, side_overflow = 0;
    // feature lattices (d > 3): keys are d shorts, the table holds a 64-bit hash of them (checked by a second hash)
    DevBuf<short> rem0s;                // [n][d+1] rounded remainders of every point (keys are rebuilt from these)
    DevBuf<unsigned char> rank8;        // [n][d+1]
    int g_d = 0;                        // ... both re-created when the feature dimension changes
    // order-preserving splat (lat_segments): the (point, remainder) incidences of the splatted points sorted by vertex,
    // within a vertex in the REFERENCE's point order (permutohedral.cpp:491-500 walks the points in order)
    DevBuf<unsigned> skeys;             // [2][cap / 2] vertex id of every incidence, before / after the sort
    DevBuf<int> svals;                  // [2][cap / 2] incidence index (point * (d+1) + remainder), before / after
    DevBuf<int> seg;                    // [2][size] first / one-past-last sorted position of every vertex
    DevBuf<char> sort_tmp;
    DevBuf<float> terms;                // [ch][n_inc] the splat's terms w * in[i] in sorted order (per filter call)
    DevBuf<int> long_list;              // vertices whose chains are longer than kLongSeg, then their count
    HostBuf<LatticeMail> mail;          // mapped, coherent host memory the resolve kernel publishes the counters in
    unsigned mail_seq = 0;
    bool count_clean = false, count2_clean = false;  // the device counters are zero (cleared by the last resolve)
    DevBuf<long long> fx;               // [(size + 1)][ch] fixed-point accumulators of the order-independent splat
                                        // (all zero between filter calls: k_fix_to_float clears what it has read)
    DevBuf<double> fx_scale;            // [32] 2^S_k, [32] 2^-S_k, then 32 unsigned: largest |value| per channel (float bits)
    const float* fx_scale_key = nullptr;  // the value array the scales were computed for ...
    int fx_scale_ch = 0;
    bool fx_scale_static = false;       // ... which the owner promises not to change (FilterReg plan: target moments)
    bool seg_valid = false;             // the arrays describe the current lattice for points >= seg_first
    int64_t seg_first = -1;
    const int* ref_pos = nullptr;       // device, may be null (identity): j-th splatted point of the reference's order ->
                                        // its position among the splatted points as the kernels store them
    DevBuf<short> kfull;                // [size][d] full key of every lattice vertex
    DevBuf<unsigned long long> gcheck;  // [size] second hash of the vertex key | 1 (0 = not yet written)
    DevBuf<float> scale_dev;            // [kMaxDG] scale factors of the embedding
};

// Build the lattice over L->feat (device, n x d float32) or L->prod.  Synchronises (the vertex count is needed on the host,
// as in the reference where get_lattice_size() drives the with_blur decision, filterreg.py:90-91).
// decide_above >= 0: the caller only wants this lattice if it has at most `decide_above` vertices.  The points are
// then embedded in two stages (1/16 of them first): the vertices of a subset are a subset of the vertices, so as
// soon as the count exceeds the threshold the answer is known and the build stops (L->built = false, L->size = a
// lower bound > decide_above) - no compaction, no neighbour tables, 15/16 of the hashing saved.
int lat_build(Lattice* L, int64_t n, int d, int with_blur, int64_t decide_above = -1);
// Decision stage of the blurred lattice into the side table, WITHOUT synchronising and without a launch of its own: 1/16
// of the points are hashed with the blur scaling (by the next lat_build's first embedding launch, side_fuse) and counted
// as they create vertices; the count is read back by that lat_build (side_pending).  A subset's vertices are a subset of
// the vertices, so side_size > threshold proves that the blurred lattice is too large.
int lat_side_stage(Lattice* L, int64_t n, int d);
// Filter `ch` channels: in [n][ch] (device) -> out [n_out][ch] (device); only points >= first are splatted
// (callers pass first > 0 only when the skipped rows are known to be zero).
// defer_slice: stop before the slice step and leave (final value plane, alpha) in L->pend_vals / L->pend_alpha - FilterReg's
// point-to-point M-step slices inside its own terms kernel (k_fr_terms<true>); whoever else needs `out` runs k_slice then.
int lat_filter(Lattice* L, const float* in, int ch, int64_t first, int64_t n_out, unsigned seq_mask, float* out,
               bool defer_slice = false);
int lat_slice(Lattice* L, const float* vals, float alpha, int ch, int64_t n_out, unsigned seq_mask, float* out);

}  // namespace prg
