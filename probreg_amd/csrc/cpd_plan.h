// Internal definition of the CPD plan (opaque `prg_cpd` of include/probreg_hip.h).
#pragma once
#include <cstddef>
#include <vector>

#include "cpd_buffers.h"
#include "prg_common.h"
#include "spd_solve.h"

// Which engine an E-step's sweeps run on while a registration is in the dense regime.  The decision needs
// sigma2, the source motion of this E-step's transform and the previous E-step's largest column minimum - all of them on
// the device - so the device takes it (last thread of k_chunk_meta_bbox) and publishes it twice: in device memory, where
// the column-pass launch the host issued AHEAD of the answer checks that it is the wanted one, and in a mapped host
// mailbox the host polls while that launch runs - no stream synchronisation, the queue never drains.
struct EngineDecision {
    unsigned seq;  // E-step counter the decision belongs to (host mailbox: written last)
    int col;       // 1: matrix-core column pass, 0: culled vector-pipe column pass
    int first;     // ... without seeds (first E-step of a registration)
    int row;       // 1: matrix-core row pass
    int fine;      // per-wave tile masks on (some groups of a chunk can be skipped by now)
    int dense;     // 0: the registration has left the dense regime for good (the host stops asking)
    float sigma2, motion, cmax, nk_ext2, nk_width, nk_far2;  // what it was decided from (PRG_DEBUG_ENGINE)
    // the switch's memory (device copy only carries it from E-step to E-step): pairs the matrix-core sweeps last evaluated
    // per owned point - targets of the column pass, source points of the row pass - and "the row pass has left them"
    float r_col, r_row;
    int row_off;
    int lean;      // 1: the matrix-core row pass runs without its residual sums (sigma2 large enough, see k_chunk_meta_bbox)
    int fused;     // 1: ONE sweep for this E-step (k_colpass_mfma<FUSED>: rigid M-step moments from the column side, no row pass)
    int deal;      // 1: a grid-mode matrix-core column launch deals its chunks interleaved (chunk c to segment c mod S): the previous
                   // sweep skipped part of its pairs.  (Also keeps the 64-bit counters behind the device copy of this struct aligned.)
};
// Device state of the engine decision: the decision itself, the matrix-core sweeps' tile counters and the LOCAL target's sums
// (prg_cpd_init_sums keeps a copy here: the caller all-reduces the moments block it also writes them to).
struct EngineState {
    EngineDecision decision;
    unsigned long long work[2];  // (128 x 16) tiles the matrix-core column / row pass evaluated (read + cleared by the decision)
    double tsum[4];              // (sum x, sum y, sum z, sum |x|^2) of the local target
};
static_assert(offsetof(EngineState, work) == sizeof(EngineDecision) && sizeof(EngineDecision) % 8 == 0,
              "the 64-bit counters sit right behind the decision");
constexpr unsigned kMailboxFlags = hipHostMallocMapped | hipHostMallocCoherent;  // how the host's copy of the decision is allocated
struct EngineArgs {  // host -> k_chunk_meta_bbox, by value
    double ext2;
    // matrix-core sweeps while they evaluate at least this many pairs per owned point (engine_leave_below, cpd_estep.hip)
    double r_col_bound, r_row_bound;  // (r_row_bound: for the lean row pass)
    double r_col_bound_fused;         // ... the dense regime's lower end while the fused single sweep may run (it competes with TWO vector-pipe sweeps)
    double r_row_bound_full;          // ... for the row pass with its residual sums (amplification above the lean factor)
    double owned_col, owned_row;  // N_local, M
    double streamed_col, streamed_row;  // M, N_local: what the count is when nothing is culled (the switch's initial memory)
    const double* tsum;           // (sum x, sum y, sum z, sum |x|^2) of the local target
    double lean_factor;           // lean row pass while mean |x|^2 / (sigma2 D) <= this
    double fused_factor;          // ... and the fused single sweep while it is <= this
    int dim;
    unsigned long long* work;     // [2] (128 x 16) tiles the matrix-core column / row pass of the PREVIOUS E-step evaluated
    float tbox[6];
    int slot, have_colmin, forced, reset;
    int deal_mode;                // PRG_MFMA_DEAL: 0 / 1 pin the chunk deal of grid-mode matrix-core column launches, -1: by the count
    double deal_below;            // ... interleaved once the previous sweep evaluated fewer than this many pairs per owned point
    int fused_allowed;            // this E-step feeds a rigid M-step and nothing else (prg_cpd_iterate / prg_cpd_set_moments_only)
    int resid_allowed;            // ... and below the matrix cores it would run as ONE residual-form sweep on the vector pipe (exact at any amplification)
    unsigned seq;
    EngineDecision* dev;
    EngineDecision* host;
};

// What the engine switch remembers from one E-step of a registration to the next (host side; EngineDecision::r_col / r_row /
// row_off are the device's share).  A default-constructed value is "a new registration starts".
struct EngineSwitch {
    bool reset = true;       // the device's share is void (new registration, engine mode changed): the next decision starts it afresh
    bool mfma_off = false;   // this registration has left the dense regime: no more engine decisions
    int pred_col = 1;        // the column-pass engine the host launches ahead of the decision (= the previous decision)
    int pred_fine = 0;       // ... and whether that decision had the per-wave tile masks on (0: dense regime -> stream mode)
    int pred_fused = 0;      // ... the previous E-step ran the fused sweep
    bool grid_fine = false;  // the previous matrix-core column pass skipped >= 10 % of its pairs: launches are cut into >= 3 rounds of shorter segments
    int deal = 0;            // ... and what the previous decision said about the chunk deal (EngineDecision::deal; the guard overrides it)
};

// Environment knobs of the CPD plan, read ONCE per process (prg::cpd_env(), cpd.hip).  Precedence everywhere: the plan's setter,
// then the environment, then the built-in default.  They exist for A/B measurements (tools/) - the defaults are the product.
//   PRG_MFMA_SEG          segments of every matrix-core launch (0: fill the chip once; pins mfma_fine_segments and the cost model)
//   PRG_MFMA_DEAL         how a grid-mode matrix-core column launch (k_colpass_mfma) deals the streamed chunks to its S segments:
//                         0: contiguous runs always, 1: interleaved (chunk c to segment c mod S) always, the all-pairs launches
//                         included; unset: interleaved once the previous sweep skipped part of its pairs (profiles/mfma_deal_ab.log)
//   PRG_MFMA_DEAL_BELOW   ... that is: evaluated fewer than this fraction of the streamed cloud per owned point (default 0.9)
//   PRG_MFMA_FINE_GRID    =0: never cut a culling matrix-core launch finer (profiles/r4_shard_window.log is the case it fixes)
//   PRG_ENGINE_RCOL/RROW  > 0: leave the matrix cores below this many evaluated pairs per owned point instead of the cost model's
//                         bound (engine_leave_below; profiles/r3_engine_switch_*.log, r4_engine_switch_*.log)
//   PRG_FUSED_RCOL_SCALE  > 0: lower end of the dense regime while a single sweep may run, as a multiple of the column pass' bound
//                         (fused_lower_bound_scale; profiles/r4_, r5_, r6_fused_lower_bound.log)
//   PRG_LEAN_FACTOR       >= 0: lean row pass while mean |x|^2 / (sigma2 D) <= this (kLeanFactor; profiles/r4_lean_error_rigid_100k_*.log)
//   PRG_FUSED_FACTOR      >= 0: replaces prg_cpd_set_fused_factor's value (fused sweep while the amplification is <= this)
//   PRG_OWNER_SWEEP       =0: no owner sweep (cpd_sweeps_owner.hip): round 5's grid / queue run the single sweep
//   PRG_DEBUG_ENGINE      set: one line per engine decision on stderr
//   PRG_SPATIAL_ORDER     morton / kd_host: the Z-curve of rounds 1 - 5 / the host build of the kd-tree order (default: device build)
// Three more are the defaults of a NEW plan and are read whenever one is created (tests/test_queue_engine_gpu.py changes them
// between plans of one process), see prg_cpd_create:
//   PRG_DENSE_ENGINE      prg_cpd_set_dense_engine's mode, clamped to [0, 2]
//   PRG_SPARSE_ENGINE     prg_cpd_set_sparse_engine's mode, clamped to [0, 2]
//   PRG_RESID_SWEEP       prg_cpd_set_resid_sweep (A/B runs of the two-sweep sparse regime)
struct CpdEnv {
    int mfma_seg = 0;
    bool fine_grid_off = false;
    int mfma_deal = -1;
    double mfma_deal_below = 0.9;
    double r_col = 0.0, r_row = 0.0;
    double fused_rcol_scale = -1.0;
    double lean_factor = -1.0, fused_factor = -1.0;
    bool owner_off = false;
    bool debug_engine = false;
    std::string spatial_order;
};

using prg::SweepQueue;  // (cpd_buffers.h)

// Communicator of the per-iteration all-reduce (comm.hip): an RCCL communicator the library created (prg_comm_create) or
// one the caller handed over (prg_comm_adopt).
struct prg_comm {
    void* nccl = nullptr;  // ncclComm_t
    int rank = 0, nranks = 1, device = 0;
    bool owned = true;     // prg_comm_destroy calls ncclCommDestroy
    int64_t calls = 0;     // all-reduces issued (tests / measurements)
};

// Every device or pinned allocation of the plan is an owning buffer (dev_buf.h): the capacity is buf.cap, and destroying the
// plan frees them.  The clouds' groups (src4, z4, rowacc, zmeta, rorig, zchunk, Mcap / tgt4, pt1, tmeta, tchunk, corig, colmin,
// Ncap) are the bases' members (cpd_buffers.h).
struct prg_cpd : prg::SourceBuffers, prg::TargetBuffers {
    int device = 0;
    hipStream_t stream = nullptr;

    int64_t M = 0, N = 0, Nglobal = 0;
    int D = 0;

    prg::DevBuf<float2> colpart;  // column pass partials [SA][Ncap] (dmin, sum); grows, never shrinks
    prg::DevBuf<float> rowpart;   // row pass partials [SB][5][Mcap] (p1, ux, uy, uz, e); grows, never shrinks
    // moment block partials [nblk][24] ... and 64 doubles of scratch at the END OF THE ALLOCATION (mom_scratch, cpd_estep.h); grows,
    // never shrinks
    prg::DevBuf<double> mompart;

    prg::DevBuf<double> state;  // PRG_NMOMENTS + PRG_NPARAMS doubles
    double* moments = nullptr;  // -> state or caller-bound memory
    double* params = nullptr;   // -> state + PRG_NMOMENTS

    // tuning (0 = auto)
    int r_col = 0, seg_col = 0, r_row = 0, seg_row = 0;

    // spatial sorting + exact culling
    bool opt_sort_src = true, opt_sort_tgt = true, opt_cull = true;
    prg::DevBuf<int> perm_src;  // [M] sorted position -> original index (empty = identity order)
    prg::DevBuf<int> perm_tgt;  // [N]
    prg::DevBuf<unsigned> motion;  // [16] float bits, slot = parity of the E-step: [0,1] max_m |z_new - z_old| of the transform,
                                // [4,5] largest column minimum of the E-step (what the host needs to decide whether the
                                // matrix-core column pass may run); [8..13] bounding box of the transformed
                                // source (lo.xyz, hi.xyz) of the current E-step
    bool have_colmin = false;
    // matrix-core (dense regime) sweeps
    bool fused_in_iterate = true;  // prg_cpd_iterate(RIGID) switches moments_only on for its own E-steps (prg_cpd_set_moments_only(2): not)
    bool moments_only = false;  // E-steps of this plan feed a RIGID M-step and nothing else: the dense regime may run the fused
                                // single sweep, which leaves no per-point p1 / px (prg_cpd_set_moments_only, prg_cpd_iterate)
    bool init_rot_orthonormal = true;  // ... only from a rotation: the column-side sums are mapped back through s R
    bool resid_sweep = true;    // ... and, where the column pass runs on the vector pipe, the residual-form single sweep (DESIGN.md 3.1f;
                                // prg_cpd_set_resid_sweep(0): two sweeps there)
    bool last_estep_fused = false;
    bool rowacc_valid = false;  // the per-point block (p1, px) holds the last E-step's result (not after a fused sweep)
    int dense_engine = 1;       // 0: VALU sweeps only, 1: matrix-core sweeps in the dense regime,
                                // 2: both sweeps on the matrix cores, always (tests)
    double dense_bound = 0.0;    // > 0: matrix-core column pass while it evaluates at least this many source points per target (0: the cost model, engine_leave_below)
    double* tsum_local = nullptr;            // -> eng_dev.p->tsum
    unsigned long long* eng_work = nullptr;  // -> eng_dev.p->work
    // (the work queues' memory - q_first_*, q*_live below - is NOT part of the switch's: a sweep over a queue sizes its units from the
    // previous sweep over that queue, whichever registration ran it)
    int q_first_col = 32, q_first_row = 32;  // groups per unit of the first queue sweep after a matrix-core one
    EngineSwitch eng;            // the engine switch's memory of this registration (prg_cpd_init_params: eng = EngineSwitch())
    prg::DevBuf<EngineState> eng_dev;        // its `decision`: device copy of the current E-step's (guard of the column-pass launches)
    prg::HostBuf<EngineDecision> eng_host;   // mapped, coherent host memory (kMailboxFlags): the mailbox the host polls
    EngineDecision* eng_host_dev = nullptr;  // ... as the device addresses it (= eng_host.dev)
    bool mfma_stream = true;    // dense-regime launches of the matrix-core sweeps are cut in stream mode (prg_cpd_set_stream_mode)
    int mfma_col_planes = 0, mfma_row_planes = 0;  // partial planes the last matrix-core column / row pass wrote (grid or stream mode)
    bool last_estep_row_lean = false;  // ... matrix-core row pass without its residual sums
    double fused_factor = 256.0;       // fused single sweep while mean |x|^2 / (sigma2 D) <= this (prg_cpd_set_fused_factor)
    double lean_factor = -1.0;         // lean row pass while mean |x|^2 / (sigma2 D) <= this (< 0: the default, 64; prg_cpd_set_lean_factor)
    bool last_estep_mfma = false, last_estep_row_mfma = false;  // engines of the last E-step's column / row pass
    double text2 = 0.0, sext2 = 0.0;  // squared bounding-box diagonals of the local target and of the source
    float tbox[6] = {0, 0, 0, 0, 0, 0};  // bounding box of the local target (lo.xyz, hi.xyz)
    // sparse regime: device-built work queues of the two sweeps; sparse_engine 1 = use them for the
    // vector-pipe sweeps of large clouds AND the owner sweep (cpd_sweeps_owner.hip) for single-sweep rigid iterations (default),
    // 0 = the grid-per-(block, segment) culled sweeps of round 1, 2 = queue always, 3 = round 5's default (1 without the owner sweep)
    SweepQueue qcol, qrow;
    int sparse_engine = 1;
    bool qcol_live = false, qrow_live = false;  // the previous E-step's column / row pass ran over the queue (its unit size adapts from there)
    // measurement hook: evaluated (wave, group) blocks per workgroup of the last culled column / row pass
    // ([0, wg_cap) column pass, [wg_cap, 2 wg_cap) row pass); wg_col / wg_row = workgroups of the last launches,
    // dense_pairs_* = pairs covered by the last NON-culled launches (0 when the culled kernels ran)
    prg::DevBuf<unsigned> wgcount;  // two halves of wg_cap(); grows, never shrinks
    int64_t wg_cap() const { return wgcount.cap / 2; }
    int64_t wg_col = 0, wg_row = 0;
    double wg_col_pairs = 128.0 * 32.0, wg_row_pairs = 128.0 * 32.0;  // pairs one counted block stands for
    double dense_pairs_col = 0.0, dense_pairs_row = 0.0;
    uint64_t estep_count = 0;   // parity selects the motion slot of the current E-step

    // staging for uploads / moments_from_estep
    prg::DevBuf<char> stage;  // grows, never shrinks (prg::ensure_stage)

    // non-rigid state
    prg::DevBuf<float> G;      // [M][M] float32 (row-major)
    prg::DevBuf<double> W;     // [M][3] float64 (row-major, 3 columns always)
    // ... or its pivoted-Cholesky factor G = F F^T (non-rigid CPD): F[k * f_ld + i], k < f_rank
    prg::DevBuf<double> F;
    int64_t f_ld = 0;          // round_up(M, 256) + 32
    int f_rank = 0, f_cap = 0;
    int nr_solver = 1;         // 1: low-rank factor when the rank allows (default), 0: dense G + M x M Cholesky
    int nr_max_rank = 0;       // 0: min(2048, M / 2)
    double nr_tol = 1.0e-11;   // the factor stops when the largest residual diagonal entry of G - F F^T is below this (the
                               // reference's own float32 G is 6e-8 from the exact kernel; 1e-11 is rank 119 at C3 - one 128-block
                               // of the reduced system - where 1e-14 is rank 176)
    double beta = 0.0;
    bool nonrigid = false;
    prg::DevBuf<double> nr_work;  // [16 M + 3 kMaxRank]: G.W product and scratch
    bool gw_valid = false;      // nr_work[0, 3M) holds G W of the current W (left by the M-step, consumed by the transform)
    prg::DevBuf<double> nr_solve;  // M-step workspace: S (fp64 M x M), block inverses, vectors; grows, never shrinks
    int* nr_info = nullptr;      // -> into nr_solve (cleared whenever that is re-created): first non-positive pivot + 1 of a low-rank M-step since the last report (0: none)
    prg::DevBuf<double> nr_prior;          // [4][M]: p1_tilde, px_tilde (3 planes) of ConstrainedNonRigidCPD
    double nr_alpha = 0.0;                 // 0 = no correspondence priors
    prg::SpdQueues nr_queues;              // the plan stream + side stream and events of the look-ahead Cholesky (spd_solve.h)

    // per-source log-weights (BCPD E-step, bcpd.py:53-72): srcw[m] = ln a_m <= 0 in kernel (sorted) order; the
    // transform kernel turns it into the additive squared distance q_m = -2 sigma2 ln a_m carried in z4.w
    prg::DevBuf<float> srcw;
    double uniform_ratio = 0.0;  // > 0: replaces M / N in the outlier constant of cpd.py:78-79
    bool bcpd = false;           // G is the inverse multiquadric kernel, W holds the displacement v_hat
    // solver of the next prg_cpd_bcpd_build_g (prg_cpd_bcpd_set_solver)
    int bcpd_solver = 0;         // 0: dense G (default), 1: factor G = F F^T or an error, 2: factor when it converges, else dense
    int bcpd_max_rank = 0;       // 0: min(2048, M / 2)
    double bcpd_tol = 1.0e-11;   // largest entry of G - F F^T the factor may leave

    prg::HostBuf<double> pinned; // 64 doubles of pinned host memory for the per-iteration parameter read-back

    bool have_source = false, have_target = false, have_estep = false;
    double last_w = 0.0;
    // z4, tgt4.w (b_n), the weights and sigma2 in PARAMS are still those of ONE E-step: set by every prg_cpd_estep, cleared by
    // whatever writes PARAMS, the weights or an E-step result of the caller's (what prg_cpd_correspond reads, cpd_correspond.hip)
    bool estep_state_live = false;
    // workspace of prg_cpd_correspond (packed clouds, partial lists, results): grows, never shrinks
    prg::DevBuf<char> corr_buf;

    // multi-GPU: when set, prg_cpd_estep / prg_cpd_init_sums end with the SUM all-reduce of the moment block (and, for a
    // non-rigid plan, of the per-point block) on the plan's stream; not owned by the plan
    prg_comm* comm = nullptr;
};

namespace prg {
struct UniqueId { char bytes[PRG_COMM_ID_BYTES]; };  // ncclUniqueId
int comm_all_reduce_f64(prg_comm* c, double* buf_dev, int64_t count, hipStream_t st);
int ensure_stage(prg_cpd* h, size_t bytes);
const CpdEnv& cpd_env();
// kd-tree order of a cloud built on the device (spatial_order.hip): pts_dev [n][dim] floats in the caller's order -> perm_dev [n]
int device_kd_order(const float* pts_dev, int64_t n, int dim, int* perm_dev, hipStream_t st, int leaf = 32);
// non-rigid (cpd_nonrigid.hip)
int nonrigid_displacement(prg_cpd* h, const double** gw_out);  // G W of the current W (device, [M][3])
int nonrigid_gw(prg_cpd* h, const double* w3, double* out3);  // out3[m][3] = G * w3[m][3] (fp64)
int nonrigid_free(prg_cpd* h);
int build_kernel_matrix(prg_cpd* h, int kind, double param);  // kind 0: rbf(beta), 1: inverse multiquadric(c)
// low-rank factor (cpd_nonrigid.hip): out[k][0..2] = sum_i F[k][i] x3[i][0..2]  /  out3[i][0..2] = sum_k F[k][i] v[k][0..2]
int lowrank_ft3(prg_cpd* h, const double* x3, double* out);
int lowrank_apply(prg_cpd* h, const double* v, double* out3);
}  // namespace prg
