/*
 * probreg_hip.h - C ABI of libprobreg_hip.so, the MI355X (gfx950) engine behind
 * probreg's CPD / FilterReg EM hot path.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the neka-nat/probreg tree, v0.3.7).  Conventions:
 *   - all functions return 0 on success, a negative prg_status on failure;
 *     prg_last_error() returns a thread-local message for the last failure;
 *   - "hd" pointers may be host OR device pointers (copied with
 *     hipMemcpyDefault); "dev" pointers must be device pointers;
 *   - point clouds are row-major (count x D) float32, D = 2 or 3;
 *   - one handle = one device = one HIP stream; calls on a handle are
 *     asynchronous on that stream unless the name ends in a host read-back
 *     (get_*, *_host) which synchronises the stream;
 *   - no torch / numpy types appear anywhere in this file.
 */
#ifndef PROBREG_HIP_H
#define PROBREG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum prg_status {
    PRG_OK = 0,
    PRG_ERR_INVALID = -1,   /* bad argument (ValueError / AssertionError in the reference) */
    PRG_ERR_HIP = -2,       /* HIP runtime error; message holds hipGetErrorString.  Also: the device of a handle (or the
                             * `device` argument) could not be selected - every entry point checks that, nothing is launched */
    PRG_ERR_STATE = -3,     /* call order violated (e.g. estep before set_target) */
    PRG_ERR_NOMEM = -4
} prg_status;

typedef enum prg_tf_kind {
    PRG_TF_RIGID = 0,       /* probreg.cpd.RigidCPD    (cpd.py:123-192) */
    PRG_TF_AFFINE = 1,      /* probreg.cpd.AffineCPD   (cpd.py:195-244) */
    PRG_TF_NONRIGID = 2     /* probreg.cpd.NonRigidCPD (cpd.py:247-303) */
} prg_tf_kind;

const char* prg_last_error(void);
int prg_version(void);
int prg_device_count(int* count);

/* ------------------------------------------------------------------------------------------
 * Layout of the two small fp64 device blocks every CPD plan owns.
 *
 * MOMENTS (PRG_NMOMENTS doubles) - the per-iteration all-reduce payload:
 *   [0]      S0   = sum_m p1_m                        (n_p,            cpd.py:88)
 *   [1..3]   Sx   = sum_m px_m                        (xp.sum(px,0),   cpd.py:169)
 *   [4..6]   Sy   = sum_m p1_m y_m                    (source.T @ p1,  cpd.py:170)
 *   [7..15]  Sxy  = sum_m px_m y_m^T   row-major 3x3  (px.T @ source,  cpd.py:173)
 *   [16..21] Syy  = sum_m p1_m y_m y_m^T  (xx,xy,xz,yy,yz,zz)          (cpd.py:179/234)
 *   [22]     Sxx  = sum_n pt1_n |x_n|^2               (cpd.py:183/237)
 *   [23]     reserved
 *   [24..26] sum_n x_n   [27] sum_n |x_n|^2   (target sums for the sigma2 initialiser,
 *                                              math_utils.py:28-29; local shard, all-reduced)
 *   [28..31] reserved (zero)
 * PARAMS (PRG_NPARAMS doubles):
 *   [0..8]   linear part, row-major 3x3: rot (rigid) or b (affine)   transformation.py:43-78
 *   [9..11]  t
 *   [12]     scale (1 for affine)
 *   [13]     sigma2        [14] q        [15] n_p of the last E-step
 *   [16]     iteration counter (as double)
 *   [17..31] reserved
 * ---------------------------------------------------------------------------------------- */
#define PRG_NMOMENTS 32
#define PRG_NPARAMS 32

typedef struct prg_cpd prg_cpd;

/* Plan life cycle.  `hip_stream` is a hipStream_t (NULL = the device's null stream).
 * Replaces: CoherentPointDrift.__init__ backend selection, cpd.py:42-59. */
int prg_cpd_create(prg_cpd** out, int device, void* hip_stream);
int prg_cpd_destroy(prg_cpd* h);

/* [r6] The order a CPD plan stores a cloud in (sorted position -> original index): the in-order walk of a left-aligned kd-tree
 * with 32-point leaves - every aligned run of 2^k leaves (the 32-point groups, 128-point blocks, 256-point chunks and 512-point
 * blocks the sweeps cull by) is one axis-aligned cell of the cloud.  on_device != 0: built on the GPU, level by
 * level (csrc/spatial_order.hip, what prg_cpd_set_source / prg_cpd_set_target run); 0: the host build (csrc/morton.h).  Both give
 * the same cells.  No reference counterpart (probreg keeps the caller's order); tests and tools. */
int prg_spatial_order(const float* points_hd, int64_t n, int dim, int on_device, int* perm_host);
/* Engine options, before the clouds are uploaded (all default to 1): Morton-sort the source / the target at
 * upload (every output keeps the caller's point order) and skip (wave, 32-point group) blocks whose every pair
 * is an exact zero in fp32.  The non-rigid path keeps the source unsorted. */
int prg_cpd_set_options(prg_cpd* h, int sort_source, int sort_target, int cull);

/* Engine of the E-step's DENSE regime (sigma2 large: every pair contributes).  mode 1 (default; clouds of >= 8192 points
 * each): the pair sweeps take their exponents from the matrix cores (bf16x3-split MFMA distance blocks)
 * while that is the faster engine - decided per E-step on the device from the number of pairs the matrix-core sweeps of
 * the previous E-step evaluated (they skip exact zeros in blocks of 512 x 256 and, per wave, 128 x 16) against a cost
 * model of the two engines; from there on the culled vector-pipe sweeps, which skip 128 x 32 blocks and share the work out
 * evenly, are faster and the registration stays on them (the row pass leaves first).  mode 0: vector-pipe sweeps only;
 * mode 2: both sweeps on the matrix cores always (tests, measurements).  bound > 0 replaces the model's bound of the
 * column pass: matrix cores while they evaluate at least `bound` source points per target; 0 keeps the current setting.
 * prg_cpd_last_estep_engine reports which engine the last E-step's column pass used (1 = matrix cores). */
int prg_cpd_set_dense_engine(prg_cpd* h, int mode, double bound);
int prg_cpd_last_estep_engine(prg_cpd* h, int* engine);
/* The bounds of that decision for a source of m points and a local target of n_local (host arithmetic, no device needed):
 * the matrix-core column pass is left below *col_bound evaluated source points per target, the row pass below *row_bound
 * evaluated targets per source point. */
int prg_cpd_engine_bounds(int64_t m, int64_t n_local, double* col_bound, double* row_bound);
/* Sparse regime (sigma2 small: most 128 x 32 blocks of P are exact zeros): 1 (default) - with M and the local N both >= 32768
 * the vector-pipe sweeps run over a device-built work queue (need-masks -> units -> persistent waves,
 * csrc/cpd_sweeps_queue.hip), smaller problems on the grid; 2 - the queue always; 0 - always one wave per (128-point block,
 * 512-point segment) whether it finds work or not (the culled sweeps of csrc/cpd_sweeps_packed.hip).  Same pairs, same
 * arithmetic, exact either way; tests / measurements.  [r6] Under mode 1 the SINGLE sweep of a rigid iteration
 * (prg_cpd_set_moments_only) is the owner sweep of csrc/cpd_sweeps_owner.hip wherever it runs on the vector pipe - the column
 * block's workgroup finds its cells through the chunk / group hierarchy of the kd-ordered clouds, no queue, no build pass
 * (DESIGN.md 3.1g); 3 - round 5's default: mode 1 without the owner sweep (the residual-form sweep over the queue / grid). */
int prg_cpd_set_sparse_engine(prg_cpd* h, int mode);
/* ... and for both sweeps of the last E-step: 1 = matrix cores, 0 = vector pipe (column pass, row pass).  An E-step that ran as a
 * single sweep (prg_cpd_last_estep_fused) has no row pass: row_engine and prg_cpd_last_estep_lean report 0 for it. */
int prg_cpd_last_estep_engines(prg_cpd* h, int* col_engine, int* row_engine);
/* 1 if the last E-step's matrix-core row pass ran WITHOUT its residual sums sum_n P_mn |x_n - o|^2 (19 instead of 21 flop
 * per pair): while sigma2 * D * 64 >= mean |x|^2 of the local target the M-step's sum_n pt1_n |x_n|^2 is taken from the column
 * side instead. */
int prg_cpd_last_estep_lean(prg_cpd* h, int* lean);
/* The amplification up to which the row pass may run lean: while mean |x|^2 / (sigma2 D) of the local target <= factor
 * (default 64; 0 = never; a huge value = wherever the matrix-core row pass runs - tests and tools/lean_error.py measure the
 * sigma2 error of the lean pass far beyond where the default allows it); negative restores the default. */
int prg_cpd_set_lean_factor(prg_cpd* h, double factor);
/* How a DENSE-regime launch of the matrix-core sweeps (nothing to skip yet) is cut into workgroups: 1 (default) - equal runs
 * of (512-point block, 256-point chunk) units over whole rounds of the workgroups the chip holds, at most one unit of
 * difference between any two; 0 - the grid of (block, segment) workgroups every other regime uses.  Same pairs, same
 * arithmetic; the partial sums are merged in a different order (tests, measurements). */
int prg_cpd_set_stream_mode(prg_cpd* h, int on);

/* Upload the (already centred) source cloud, replicated on every device.
 * Replaces: CoherentPointDrift.set_source, cpd.py:61-62. */
int prg_cpd_set_source(prg_cpd* h, const float* source_hd, int64_t m, int dim);

/* Upload this device's contiguous shard of the target cloud; n_global is the number of
 * target points over all shards (it enters `c`, cpd.py:78-79, and q0, cpd.py:148).
 * Replaces: the `target` argument of CoherentPointDrift.registration, cpd.py:106. */
int prg_cpd_set_target(prg_cpd* h, const float* target_hd, int64_t n_local, int dim, int64_t n_global);

/* Optional: make the plan accumulate its moments into caller-owned device memory
 * (PRG_NMOMENTS doubles) so the caller can all-reduce them in place (RCCL). */
int prg_cpd_bind_moments(prg_cpd* h, double* moments_dev);
/* Device addresses of the blocks (for in-place collectives / zero-copy views). */
int prg_cpd_moments_ptr(prg_cpd* h, double** moments_dev);
int prg_cpd_params_ptr(prg_cpd* h, double** params_dev);

/* ---- multi-GPU: the one exchange step of the path ---------------------------------------------
 * The reference is single-process (its EM loop, cpd.py:106-120, is what gets sharded): every rank keeps the whole
 * source, owns a run of target rows, and the partial MOMENTS of its E-step (cpd.py:84-88 restricted to its columns)
 * are summed over the ranks before the M-step (cpd.py:160-192 / 219-244), which every rank then runs identically.
 * A prg_comm wraps an RCCL communicator (librccl is bound with dlopen on first use - a single-GPU caller never
 * loads it): rank 0 calls prg_comm_unique_id and hands the PRG_COMM_ID_BYTES bytes to the other ranks by any means
 * (the Python layer broadcasts them through torch.distributed), every rank calls prg_comm_create (ncclCommInitRank;
 * collective).  prg_comm_adopt wraps an ncclComm_t the caller already has (not destroyed by prg_comm_destroy).
 * With prg_cpd_set_comm(plan, comm) the plan's prg_cpd_init_sums and prg_cpd_estep END with the SUM all-reduce of
 * MOMENTS (init_sums: all 32 doubles; an E-step: the 24 it wrote; a non-rigid plan: the per-point block of prg_cpd_rowacc_ptr as well) on the plan's own stream: an EM
 * iteration is enqueue-only, nothing between the E-step's last kernel and the M-step leaves the library.
 * comm == NULL detaches (the caller all-reduces MOMENTS itself, e.g. through prg_cpd_bind_moments). */
#define PRG_COMM_ID_BYTES 128
typedef struct prg_comm prg_comm;
int prg_comm_available(int* rccl_version);            /* PRG_OK when librccl could be bound (version: ncclGetVersion) */
int prg_comm_unique_id(unsigned char* id_out);        /* [PRG_COMM_ID_BYTES], host */
int prg_comm_create(prg_comm** out, const unsigned char* id, int rank, int nranks, int device);
int prg_comm_adopt(prg_comm** out, void* nccl_comm, int device);
int prg_comm_info(prg_comm* c, int* rank, int* nranks, int64_t* all_reduces_issued);
int prg_comm_destroy(prg_comm* c);
/* In-place SUM all-reduce of `count` doubles at a device address, on `hip_stream` (what the plan issues itself). */
int prg_comm_all_reduce_f64(prg_comm* c, double* buf_dev, int64_t count, void* hip_stream);
int prg_cpd_set_comm(prg_cpd* h, prg_comm* comm);
/* `n_iter` EM iterations of the rigid / affine registration enqueued back to back: transform + E-step [+ all-reduce]
 * + M-step, the loop body of CoherentPointDrift.registration (cpd.py:110-113) without its host-side convergence test
 * (tol < 0, no callbacks).  Nothing is read back; prg_cpd_get_params afterwards synchronises. */
int prg_cpd_iterate(prg_cpd* h, int kind, int update_scale, double w, int n_iter);
/* What a RIGID EM iteration needs of its E-step (cpd.py:160-192) are 23 sums, not the per-point arrays p1 / px.  mode 1: every
 * prg_cpd_estep of this plan may therefore run, while sigma2 is large (dense regime, sigma2's amplification within the fused
 * factor), as ONE sweep over the pairs - the column pass with the row pass' contraction on the source side, the moments taken
 * from per-column sums - instead of two: MOMENTS, pt1 and the parameter block come out as always,
 * prg_cpd_get_estep has no p1 / px to return after such an E-step (it says so), and the caller must follow it with
 * prg_cpd_mstep(PRG_TF_RIGID).  mode 0 (default): only prg_cpd_iterate(PRG_TF_RIGID) does this, for its own E-steps.
 * mode 2: nobody does (two sweeps always: tests, measurements).  prg_cpd_last_estep_fused reports what the last E-step did. */
int prg_cpd_set_moments_only(prg_cpd* h, int mode);
int prg_cpd_last_estep_fused(prg_cpd* h, int* fused);
/* The fused sweep runs while the matrix-core column pass would and mean |x|^2 / (sigma2 D) of the local target <= factor
 * (default 256: sigma2 within 1.4e-6 of the fp64 oracle's there, within 3e-6 at 1300 - profiles/r4_fused_error_100k.log);
 * tests force it further with a huge value, 0 switches it off. */
int prg_cpd_set_fused_factor(prg_cpd* h, double factor);
/* Below the dense regime (column pass on the vector pipe) the same E-steps - those that feed nothing but a rigid M-step,
 * cpd.py:160-192 - run as ONE sweep as well: the culled / queued column pass carries the residual sums of its columns,
 * U_n = sum_m K (x_n - z_m) and R_n = sum_m K |x_n - z_m|^2, and the moments follow per column in fp64 (no
 * amplification limit: the sums are residuals against the current transformation).  on = 1 (default) / 0: two sweeps there
 * (A/B measurements, tests).  prg_cpd_last_estep_fused reports 1 for either single sweep, prg_cpd_last_estep_engine which pipe
 * its column pass ran on. */
int prg_cpd_set_resid_sweep(prg_cpd* h, int on);

/* sigma2 initialiser, step 1: local target sums -> MOMENTS[24..27] (others zeroed).
 * Replaces: mu.squared_kernel_sum, math_utils.py:28-29 -> cc/math_utils.cc:5-15
 * (closed form, never materialises M x N). All-reduce MOMENTS between step 1 and 2. */
int prg_cpd_init_sums(prg_cpd* h);
/* step 2: sigma2_0 and q0 = 1 + N*D/2*log(sigma2_0) into PARAMS.  `init_params_host` (NULL = identity,
 * zero, 1, zero) holds 16 doubles: [0..8] linear part, [9..11] t, [12] scale, [13..15] delta =
 * origin_target - origin_source when the caller subtracted different origins from the two uploaded
 * clouds (sigma2_0 is a mean squared source-target distance and is not invariant to that).
 * Replaces: RigidCPD._initialize cpd.py:145-153, AffineCPD._initialize :209-217,
 * NonRigidCPD._initialize :277-282. */
int prg_cpd_init_params(prg_cpd* h, const double* init_params_host);

/* One E-step on the local shard with the transformation currently in PARAMS:
 * transform (transformation.py:49-50 / 77-78 / 101-102), column pass (den, cpd.py:74-82),
 * row pass (P1, PX in residual form, cpd.py:84-87) and the fp64 moment reduction.
 * Result: MOMENTS[0..22] (local partial sums).  `w` is the uniform-noise weight.
 * Replaces: CoherentPointDrift.expectation_step, cpd.py:71-88. */
int prg_cpd_estep(prg_cpd* h, double w);

/* Same E-step with HIP events recorded on the plan's stream between its kernels.
 * ms_out[0..4] = transform, column pass, column finalise, row pass, moment reduction; ms_out[5] = total.
 * (measurement hook for bench.py's `roofline` object; synchronises the stream) */
int prg_cpd_estep_timed(prg_cpd* h, double w, float* ms_out);

/* Measurement hook: source-target pairs the column / row pass of the LAST E-step actually evaluated.  The culled
 * sweeps skip (wave, 32-point group) blocks whose every pair is an exact zero; each workgroup
 * leaves its count of evaluated blocks (128 x 32 pairs each) in a device array that is summed here.  Dense
 * launches report the pairs their grid covers (pads included).  Synchronises the stream. */
int prg_cpd_pair_counts(prg_cpd* h, double* col_pairs, double* row_pairs);

/* M-step from (all-reduced) MOMENTS into PARAMS; identical on every rank.
 * Replaces: RigidCPD._maximization_step cpd.py:160-192 (update_scale as there) and
 * AffineCPD._maximization_step cpd.py:219-244. */
int prg_cpd_mstep(prg_cpd* h, int kind, int update_scale);

/* Host read-back / overwrite of PARAMS (synchronises the stream). */
int prg_cpd_get_params(prg_cpd* h, double* params_host);
int prg_cpd_set_params(prg_cpd* h, const double* params_host);
int prg_cpd_get_moments(prg_cpd* h, double* moments_host);

/* Materialise the EstepResult of the last prg_cpd_estep in the reference's terms
 * (cpd.py:17, :84-88): pt1[n_local], p1[m], px[m*dim] as float64; any pointer may be NULL.
 * p1 / px are this shard's partial sums over its local target points. */
int prg_cpd_get_estep(prg_cpd* h, double* pt1_hd, double* p1_hd, double* px_hd);
/* Transformed source (m x dim, float32) used by the last E-step. */
int prg_cpd_get_tsource(prg_cpd* h, float* tsource_hd);

/* M-step from explicitly supplied EstepResult arrays (the reference's public
 * maximization_step(target, estep_res) signature, cpd.py:90-93): uploads pt1/p1/px
 * (float64, host or device, caller's point order), rebuilds MOMENTS[0..22] on the device and the
 * per-point (p1, px) block the non-rigid solve reads (NonRigidCPD.maximization_step, cpd.py:272-303:
 * follow with prg_cpd_set_params(sigma2_p) and prg_cpd_mstep_nonrigid); no M-step yet. */
int prg_cpd_moments_from_estep(prg_cpd* h, const double* pt1_hd, const double* p1_hd, const double* px_hd);

/* Tuning knobs (0 keeps the automatic value): points per lane (2 or 4 select the non-culled packed sweeps, -2 / -4
 * their scalar form; 0 = automatic, which is also the only setting that uses the culled sweeps) and the number of
 * segments (<= 256) the streamed axis is split into, for the column and the row pass.  The culled sweeps evaluate
 * four consecutive segments per workgroup, so S segments occupy ceil(S / 4) partial planes. */
int prg_cpd_set_tuning(prg_cpd* h, int r_col, int seg_col, int r_row, int seg_row);

/* ---- non-rigid CPD ------------------------------------------------------------------- */
/* Build G_ij = exp(-|y_i-y_j|^2/(2*beta)) once per source.
 * Replaces: NonRigidTransformation.__init__ transformation.py:91-99 -> mu.rbf_kernel
 * math_utils.py:36-37 -> cc/math_utils.cc:17-19.
 * The plan does not store the M x M matrix when it does not have to: a Gaussian kernel matrix of a point cloud is
 * numerically low rank, and the plan keeps its pivoted-Cholesky factor G = F F^T (fp64, M x r, columns evaluated on the
 * fly; the factorisation stops when every entry of G - F F^T is below `tol`, default 1e-11 - the reference's float32 G is
 * 6e-8 from the exact kernel).  Every later product with
 * G and the M-step's solve then cost O(M r) / O(M r^2).  When the rank would exceed max_rank the plan
 * falls back to the dense float32 matrix and the M x M fp64 Cholesky. */
int prg_cpd_nonrigid_build_g(prg_cpd* h, double beta);
/* Solver of the next prg_cpd_nonrigid_build_g.  mode 1 (default): low-rank factor when the rank allows; mode 0: always
 * the dense matrix.  max_rank: 0 = min(2048, M / 2); tol: 0 keeps the current value. */
int prg_cpd_nonrigid_set_solver(prg_cpd* h, int mode, int max_rank, double tol);
/* Rank of the factor the plan holds (0: it holds the dense matrix). */
int prg_cpd_nonrigid_rank(prg_cpd* h, int* rank);
/* Copy G (m*m float32, row-major) out - parity tests / `tf.g` attribute (evaluated on the spot when the plan holds only
 * the factor). */
int prg_cpd_nonrigid_get_g(prg_cpd* h, float* g_hd);
/* Set / get W (m x dim float64).  W = 0 after build_g (cpd.py:281). */
int prg_cpd_nonrigid_set_w(prg_cpd* h, const double* w_hd);
int prg_cpd_nonrigid_get_w(prg_cpd* h, double* w_hd);
/* T = Y + G W for the current W (m x dim float64): NonRigidTransformation._transform on the control
 * points, transformation.py:101-102. */
int prg_cpd_nonrigid_apply(prg_cpd* h, double* t_hd);
/* Correspondence priors of ConstrainedNonRigidCPD (cpd.py:306-404): p1_tilde [m] and px_tilde [m x dim]
 * (float64) are the row sums / target-weighted row sums of the 0-1 prior matrix, `alpha` its reliability;
 * the next prg_cpd_mstep_nonrigid then solves cpd.py:391-396.  NULL pointers clear the priors. */
int prg_cpd_nonrigid_set_priors(prg_cpd* h, const double* p1_tilde_hd, const double* px_tilde_hd, double alpha);
/* Device address of the per-point E-step block (4*m doubles: p1[m], px0[m], px1[m], px2[m])
 * followed by MOMENTS-style scalars; this is the non-rigid all-reduce payload. */
int prg_cpd_rowacc_ptr(prg_cpd* h, double** rowacc_dev, int64_t* count);
/* Non-rigid M-step: W = solve(diag(p1) G + lmd*sigma2_prev*I, px - diag(p1) Y), T = Y + G W,
 * sigma2 = (tr(X^T diag(pt1) X) - 2 tr(px^T T) + tr(T^T diag(p1) T)) / (n_p D), q := sigma2.
 * Replaces: NonRigidCPD._maximization_step, cpd.py:284-303. */
int prg_cpd_mstep_nonrigid(prg_cpd* h, double lmd);

/* ---- Bayesian CPD -------------------------------------------------- */
/* Per-source weights of the E-step: P_mn = a_m e_mn / (c + sum_m a_m e_mn), e_mn = exp(-|x_n - z_m|^2 / 2 sigma2),
 * with a_m = exp(log_weights[m]), log_weights <= 0 ([m] float64, host or device, caller's point order); NULL
 * clears them.  `uniform_ratio` > 0 replaces M/N in the outlier constant c = (2 pi sigma2)^(D/2) w/(1-w) * ratio.
 * BCPD's E-step (bcpd.py:53-72) is this with a_m = alpha_m exp(-s^2 D Sigma_mm / 2 sigma2) and ratio = 1/N
 * (both rescaled by max a_m on the host); nu' = pt1, nu = p1, px come from prg_cpd_get_estep as for CPD.
 * Replaces: BayesianCoherentPointDrift.expectation_step, bcpd.py:53-72 (the M x N `pmat`, its `np.kron`
 * products :69-70 and the Python list comprehension :57). */
int prg_cpd_set_source_weights(prg_cpd* h, const double* log_weights_hd, double uniform_ratio);
/* G = inverse multiquadric kernel 1/sqrt(|y_i - y_j|^2 + c) of the source in float32 (cc/math_utils.cc:32-34,
 * bcpd.py:107) and BCPD mode: the transform becomes z = s R (y + v_hat) + t (CombinedTransformation) with the
 * v_hat of the last prg_cpd_bcpd_solve (0 before the first). */
int prg_cpd_bcpd_build_g(prg_cpd* h, double c);
/* How the next prg_cpd_bcpd_build_g holds the coherence kernel of bcpd.py:107 and how prg_cpd_bcpd_solve then evaluates
 * bcpd.py:123-129 (no counterpart in the reference, which always forms the M x M matrix and inverts it twice):
 *   mode 0 (default)  the dense float32 matrix and the M x M fp64 Cholesky below;
 *   mode 1            the pivoted-Cholesky factor G = F F^T (fp64, M x r, every entry of G - F F^T <= tol) and an r x r
 *                     solve, O(M r^2) per M-step and no M x M array at all; prg_cpd_bcpd_build_g fails with
 *                     PRG_ERR_INVALID, naming the rank and the residual reached, when tol is not met within max_rank -
 *                     a cloud much larger than the coherence length sqrt(c) has no such factor;
 *   mode 2            the factor when it converges, the dense matrix otherwise.
 * max_rank: 0 = min(2048, M / 2), otherwise at most 2048 (and M); tol: 0 = 1e-11.  prg_cpd_nonrigid_rank reports the
 * rank of the factor a BCPD plan holds (0: dense).  The factor truncates G: the results move by about
 * cfac * nu * tol / lmd relative, so tol has to stay small against lmd / (cfac * nu). */
int prg_cpd_bcpd_set_solver(prg_cpd* h, int mode, int max_rank, double tol);
/* Core of CombinedBCPD._maximization_step (bcpd.py:123-133) for nu = nu_hd ([m] float64, caller's order) or, when
 * nu_hd is NULL, the p1 of the last E-step:
 *   Sigma = (lmd G^-1 + cfac diag(nu))^-1,  v_hat = cfac * Sigma * diag(nu) * resid   (resid = T^-1(x_hat) - y),
 * returned as v_hat [m x dim] and diag(Sigma) [m] (float64, caller's point order); v_hat also stays on the
 * device for the next transform.  Woodbury form on S = (lmd/cfac) I + D^1/2 G D^1/2 - no G^-1, no M x M inverse:
 * fp64 Cholesky + a triangular solve with M right-hand sides on the matrix cores (4/3 M^3 flop).
 * On a plan that holds the factor (prg_cpd_bcpd_set_solver): Sigma = F A^-1 F^T / lmd with the r x r matrix
 * A = I + (cfac/lmd) F^T D F = L L^T, v_hat = (cfac/lmd) F A^-1 F^T D resid and Sigma_mm = |L^-1 f_m|^2 / lmd. */
int prg_cpd_bcpd_solve(prg_cpd* h, double lmd, double cfac, const double* nu_hd, const double* resid_hd,
                       double* vhat_hd, double* sigma_diag_hd);

/* ---- direct Gauss transform ------------------------------------------------------------ */
/* out[c*t + i] = sum_j weights[c*s + j] * exp(-|target_i - source_j|^2 / h^2), float64 out.
 * Unlike the CPD clouds these are FLOAT64 (row-major count x dim): the reference's direct path works on the arrays as
 * given (float64), and a narrow kernel is sensitive to the rounding of the coordinates - the differences are formed in
 * fp64, distance and exponential in fp32, weights and sums in fp64; up to four weight rows share one sweep.
 * Replaces: gauss_transform._gauss_transform_direct / Direct.compute / GaussTransform.compute
 * (gauss_transform.py:10-25, 46-60). */
int prg_gauss_transform_direct(int device, void* hip_stream, const double* source_hd, int64_t s,
                               const double* target_hd, int64_t t, int dim, const double* weights_hd,
                               int n_weight_rows, double h, double* out_hd);
/* The same sum with squared distance, exponential and accumulation in fp64 (prg_gauss_transform_direct takes the
 * exponential in fp32): the K x K component pairs of cost_functions.py:36-41 inside the GMMReg cost functions
 * (cost_functions.py:57-65, 89-102), where BFGS differentiates the result. */
int prg_gauss_transform_direct_f64(int device, void* hip_stream, const double* source_hd, int64_t s,
                               const double* target_hd, int64_t t, int dim, const double* weights_hd,
                               int n_weight_rows, double h, double* out_hd);

/* sum_{m,n} |x_m - y_n|^2 / (M*D*N), closed form in fp64 on the device: (n sum|x|^2 + m sum|y|^2 - 2 sum x . sum y) / (M*D*N)
 * over fp64 clouds of any dim in [1, 64].  The three terms cancel: the result is good to about 1e-16 x (their size / the result),
 * so the caller passes clouds it has moved near the origin by one common point (the quantity is a sum of differences and does
 * not change); probreg_amd.math_utils.squared_kernel_sum subtracts the mean of all points in fp64.
 * Replaces: mu.squared_kernel_sum, math_utils.py:28-29. */
int prg_squared_kernel_sum(int device, void* hip_stream, const double* x_hd, int64_t m,
                           const double* y_hd, int64_t n, int dim, double* out_host);
/* Dense K = exp(-|x_i-y_j|^2/(2*beta)) float32 (rows = x). Replaces mu.rbf_kernel, math_utils.py:36-37. */
int prg_rbf_kernel(int device, void* hip_stream, const float* x_hd, int64_t m, const float* y_hd,
                   int64_t n, int dim, double beta, float* out_hd);
/* Dense K = 1/sqrt(|x_i-y_j|^2 + c) float32 (rows = x).  Replaces mu.inverse_multiquadric_kernel,
 * math_utils.py:50-51 -> cc/math_utils.cc:32-34 (BCPD's coherence kernel, bcpd.py:107). */
int prg_inverse_multiquadric_kernel(int device, void* hip_stream, const float* x_hd, int64_t m, const float* y_hd,
                                    int64_t n, int dim, double c, float* out_hd);
/* mean_i min_j |a_i - b_j| by brute force on the GPU (float32 distances, float64 mean).
 * Replaces mu.compute_rmse, math_utils.py:32-33 (cKDTree query; BCPD's convergence criterion bcpd.py:93). */
int prg_nn_mean_distance(int device, void* hip_stream, const float* a_hd, int64_t m, const float* b_hd, int64_t n,
                         int dim, double* out_host);

/* ---- CPD correspondences: top-k posterior matches per point (csrc/cpd_correspond.hip) ---- */
/* No reference counterpart: the reference hands back a transformation only; a user of it forms the dense M x N matrix P of
 * cpd.py:84 on small clouds and takes an argmax.  Here P is never formed; the matches come from one sweep over all pairs in the
 * log domain, s_mn = log2 P_mn = b_n - kappa (|x_n - z_m|^2 + q_m), kappa = log2(e) / (2 sigma2).
 *
 * The plan-free stage: for each of the n_o owned points ([n_o][dim] float32, dim 2 or 3) the k streamed points with the largest
 *   score = owned_bias + streamed_bias - kappa |owned - streamed|^2      (float32; differences formed before squaring)
 * in descending order; scores that are equal as float32 rank by the smaller streamed index.  Either bias ([n] float32) may be
 * NULL, meaning 0: with both NULL this is an exact k-nearest-neighbour search.  1 <= k <= 8 and k <= n_s.  `segments` cuts the
 * streamed cloud into that many pieces swept by separate workgroups (0: automatic, at most 4096); the result does not depend on
 * it, bit for bit.  index_out / score_out: [n_o][k] int32 / float32.  All arrays host or device.  A pair whose score is NaN
 * (a NaN coordinate or bias) is never listed; a row that fewer than k pairs can fill ends in index -1, score -inf. */
int prg_topk_sweep(int device, void* hip_stream, const float* owned_hd, const float* owned_bias_hd, const float* streamed_hd,
                   const float* streamed_bias_hd, int64_t n_o, int64_t n_s, int dim, double kappa, int k, int segments,
                   int* index_out_hd, float* score_out_hd);
/* On a plan, after prg_cpd_estep: side 0 - for every source point m the k target points n with the largest s_mn; side 1 - for
 * every target point n the k source points m.  Rows and entries are in the caller's point order, equal scores rank by the smaller
 * caller index (the plan's internal order never shows).  index_out [owned][k] int32, log2_prob_out [owned][k] float32 (the score as
 * computed), prob_out [owned][k] float64 (exp2 of it; may underflow to 0 while the score stays finite) - host arrays, the last two
 * may be NULL.  A column whose denominator underflowed takes den = float32 eps + c, as cpd.py:81-82.
 * Reads what the E-step left: the transformed source with q_m (z4), b_n = -log2(den_n + c) (tgt4.w) and sigma2 in PARAMS.  Every
 * form of the E-step - the two sweeps, the fused single sweep on the matrix cores and the residual-form single sweep - writes
 * b_n, so any of them will do here (p1 for the source side's mass exists after the two sweeps only).  PRG_ERR_STATE when no E-step
 * has run, or when the plan has moved on since (prg_cpd_mstep / _mstep_nonrigid / _iterate, prg_cpd_set_params / _init_params,
 * prg_cpd_set_source_weights, prg_cpd_moments_from_estep, new clouds): b_n would belong to another sigma2.  PRG_ERR_STATE on a
 * plan whose target is sharded over ranks (n_local != n_global).  A caller that writes PARAMS through prg_cpd_params_ptr is
 * invisible to that check and has to run prg_cpd_estep again itself.  Pairs with a NaN score are never listed (index -1,
 * score -inf fill such a row), as in prg_topk_sweep. */
int prg_cpd_correspond(prg_cpd* h, int side, int k, int* index_out, float* log2_prob_out, double* prob_out);
/* Host only: owned points per workgroup of the sweep (one per lane) and streamed points per trip of its loop. */
int prg_cpd_correspond_tile_shape(int* owned_per_workgroup, int* streamed_per_tile);

/* ---- CPD batch plan: many small rigid / affine registrations per launch (csrc/cpd_batch.hip) ---- */
/* Replaces a host loop over registration_cpd (cpd.py:407-456), i.e. B runs of the EM driver cpd.py:106-120, by one plan whose
 * launch count per EM iteration does not depend on B; the reference has no batched interface.  Problem b keeps the semantics of
 * its own registration: closed-form sigma2 initialiser and q0 (cpd.py:145-153 / 209-217), E-step cpd.py:71-88, M-step
 * cpd.py:160-192 / 219-244, and the convergence test |q - q_prev| < tol_b of cpd.py:115-117, taken on the device. */
typedef struct prg_cpd_batch prg_cpd_batch;
/* Host only: the tile width (target columns per sweep workgroup) and the source-chunk length of the batch sweep. */
int prg_cpd_batch_tile_shape(int* tile_columns, int* source_chunk);
/* Host only: the sweep's tile table for problems of m[b] source and n[b] target points, as (problem, first column, column count)
 * triples in launch order; *ntiles is their number, tiles_out (may be NULL) receives up to `capacity` of them.  A problem's tiles
 * depend on its own sizes only. */
int prg_cpd_batch_tile_table(int nb, const int64_t* m, const int64_t* n, int* tiles_out, int64_t capacity, int64_t* ntiles);
/* nb problems in `dim` dimensions: problem b owns source points [source_offsets[b], source_offsets[b+1]) of the packed host array
 * `sources` ([total][dim] doubles) and the same for the target.  The caller has centred every cloud on its own fp64 mean, as
 * cpd.py of this project does for one problem (the points are stored as fp32). */
int prg_cpd_batch_create(prg_cpd_batch** out, int device, void* hip_stream, int dim, int nb, const int64_t* source_offsets,
                         const int64_t* target_offsets, const double* sources, const double* targets);
int prg_cpd_batch_destroy(prg_cpd_batch* h);
/* (Re)starts every registration: sigma2_0, q_0 (cpd.py:145-153) and the initial transform of every problem in one launch.
 * init_params_host: NULL (identity) or [nb][16] doubles, per problem PARAMS[0..12] followed by delta = origin_target -
 * origin_source (the layout prg_cpd_init_params takes for one problem; a rigid problem's linear part must be a rotation). */
int prg_cpd_batch_init(prg_cpd_batch* h, const double* init_params_host);
/* Up to n_iter EM iterations (cpd.py:110-117) of every problem still running, two launches per iteration for the whole batch.
 * w[nb], tol[nb]: host arrays.  A problem stops after the M-step at which |q - q_prev| < tol[b] (the first comparison is against
 * q_0) and is frozen from then on; tol[b] < 0 never stops.  With every tol[b] < 0 the call only enqueues; otherwise the host reads
 * the number of running problems once every 8 iterations and stops enqueuing at 0. */
int prg_cpd_batch_iterate(prg_cpd_batch* h, int kind, int update_scale, const double* w, const double* tol, int n_iter);
/* Number of problems that have not stopped (synchronises). */
int prg_cpd_batch_active(prg_cpd_batch* h, int* active);
/* [nb][PRG_NPARAMS] parameter blocks (centred frames) and, if n_iter_host is not NULL, the EM iterations every problem ran
 * (synchronises).  Replaces reading MstepResult cpd.py:18 of every registration. */
int prg_cpd_batch_get_params(prg_cpd_batch* h, double* params_host, int* n_iter_host);

/* ---- permutohedral lattice (Gaussian filtering) --------------------------------------------- */
/* Replaces the pybind class probreg._permutohedral_lattice.Permutohedral
 * (cc/permutohedral_lattice_py.cc:13-21 over third_party/permutohedral/permutohedral.cpp) behind
 * probreg.gaussian_filtering.Permutohedral (gaussian_filtering.py:8-17). */
typedef struct prg_ph prg_ph;
/* How the splat (permutohedral.cpp:491-500 / :548-556, `values[o] += w * in[i]` over the points in order) accumulates,
 * process-wide, for prg_ph_filter and prg_fr_estep:
 *   1 (default)  64-bit fixed-point atomics: order independent - identical bits from run to run, every vertex the correctly
 *                rounded exact sum of its terms (the reference's float32 chain carries its own round-off; the two agree to it);
 *   2            the reference's own order: one sequential float32 chain per vertex in point order (stable sort of the
 *                point-vertex incidences by vertex, then the chains) - the reference's BITS, at the price of the sort and of
 *                chains as long as the busiest vertex has points;
 *   0            float atomics in arrival order (round-off level run-to-run noise; the measurement baseline). */
int prg_lattice_set_splat_mode(int mode);
int prg_ph_create(prg_ph** out, int device, void* hip_stream);
int prg_ph_destroy(prg_ph* h);
/* init(features, with_blur): points is n x d row-major float32 (the reference passes the transpose). */
int prg_ph_init(prg_ph* h, const float* points_hd, int64_t n, int dim, int with_blur);
/* get_lattice_size() */
int prg_ph_lattice_size(prg_ph* h, int* size);
/* filter(v, start): values n x channels row-major float32 -> out, same shape.  `start` does not exist
 * here because the reference drops it (permutohedral.cpp:608-616). */
int prg_ph_filter(prg_ph* h, const float* values_hd, int channels, float* out_hd);

/* ---- FilterReg rigid point-to-point ------------------------------------------------------------ */
typedef struct prg_filterreg prg_filterreg;
int prg_fr_create(prg_filterreg** out, int device, void* hip_stream);
int prg_fr_destroy(prg_filterreg* h);
/* Clouds as float64 (the reference transforms / scales in float64 before the float32 lattice cast).
 * Replaces: RigidFilterReg(source=...) filterreg.py:150-156 and the `target` of registration, :120. */
int prg_fr_set_source(prg_filterreg* h, const double* source_hd, int64_t m, int dim);
int prg_fr_set_target(prg_filterreg* h, const double* target_hd, int64_t n, int dim);
/* Current rigid transform (rot: row-major 3x3 with the dim x dim block filled, t: 3) and sigma2. */
int prg_fr_set_state(prg_filterreg* h, const double* rot9, const double* t3, double sigma2);
/* E-step: transform the source, build the lattice over [t_source; target] / sigma (rebuilt without blur
 * when it has more than n*alpha vertices), filter (1 | target | |target|^2) and keep the first m rows.
 * Replaces: FilterReg.expectation_step, filterreg.py:78-108 (pt2pt). */
int prg_fr_estep(prg_filterreg* h, double alpha, int* lattice_size, int* with_blur);
/* m0 [m], m1 [m x dim], m2 [m] of the last E-step (float32; any pointer may be NULL). */
int prg_fr_get_estep(prg_filterreg* h, float* m0_hd, float* m1_hd, float* m2_hd);
/* M-step (weighted Kabsch + composition + optional sigma2 update).  out_host[18]: [0..8] rot, [9..11] t,
 * [12] sigma2 of the NEXT iteration, [13] q, [14] number of points with m0 != 0, [15] new (un-clamped) sigma2,
 * [16] 1 if a transform was estimated (0 = every m0 was zero: the reference returns q = None,
 * filterreg.py:167-168), [17] sigma2 this step used.  min_sigma2 >= 0 advances the device state like the driver
 * (`self._sigma2 = max(res.sigma2, min_sigma2)`, filterreg.py:140) so the loop needs no upload per iteration;
 * a negative min_sigma2 leaves the device sigma2 untouched (M-step only).  out_host may be NULL: the M-step is only
 * enqueued, nothing is read back and the host does not wait (a driver with a fixed iteration count and no callbacks
 * reads the state once at the end, prg_fr_get_state).
 * Replaces: RigidFilterReg._maximization_step filterreg.py:158-196 + cc/kabsch.cc:6-109. */
int prg_fr_mstep(prg_filterreg* h, double w, int update_sigma2, double min_sigma2, double* out_host);
/* The device state (synchronises): out_host[20] = the 18 entries of prg_fr_mstep, then [18] q of the last M-step that had
 * anything to fit (an all-zero one sets [13] to NaN and [16] to 0), [19] the number of such M-steps since prg_fr_set_state. */
int prg_fr_get_state(prg_filterreg* h, double* out_host);
/* How the last prg_fr_estep / prg_fr_kinematic_estep on the plan chose between the blurred and the non-blurred lattice
 * (filterreg.py:90-91; the choice itself is the reference's every time).  Host bookkeeping, nothing is launched or copied.
 * out4[0] route: 1 blurred lattice built first and kept, 2 built first and rejected (the previous E-step blurred, or the
 *   threshold N * alpha is negative or >= 2e9), 3 non-blurred lattice built while a 1/16 sample proved the blurred one too
 *   large, 4 blurred build with the threshold stopped after its first sixteenth, 5 that build completed and kept,
 *   6 completed and rejected;
 * out4[1] lattice builds of the E-step (1..3); out4[2] hash-table attempts of its last build (2: retried at full capacity);
 * out4[3] 1 if routes 3..6 looked at a sixteenth of the points first (M + N >= 4096), else 0.
 * PRG_ERR_STATE before the first E-step, and after one that failed.  No reference counterpart: tests and diagnosis. */
int prg_fr_last_route(prg_filterreg* h, int* out4);

/* Point-to-plane objective (filterreg.py:101-105, 183-186): target normals (n x 3 float64, NULL clears) add a
 * 3-channel filter `nx` to the E-step; prg_fr_mstep_pt2pl solves the 6 x 6 twist system
 * (cc/point_to_plane.cc:6-32), applies se3_op.twist_mul (se3_op.py:44-56); out_host as prg_fr_mstep with
 * [13] q = sum w^2 residual^2. */
int prg_fr_set_target_normals(prg_filterreg* h, const double* normals_hd);
int prg_fr_get_nx(prg_filterreg* h, float* nx_hd);
int prg_fr_mstep_pt2pl(prg_filterreg* h, double w, int update_sigma2, double min_sigma2, double* out_host);

/* M-step from caller-supplied E-step arrays - the reference's public FilterReg.maximization_step(t_source, target,
 * estep_res, w, objective_type) -> RigidFilterReg._maximization_step (filterreg.py:110-113, 158-196).  No handle:
 * t_source [m x dim] float64; m0 [m], m1 [m x dim], m2 [m] (NULL = sigma2 is not re-estimated, filterreg.py:190),
 * nx [m x 3] (non-NULL selects the point-to-plane objective, filterreg.py:183-186) float32; n_target enters the
 * outlier constant (filterreg.py:164); rot9 / t3 / sigma2 = trans_p and the current variance.  out_host[18] as
 * prg_fr_mstep ([12] repeats the input sigma2, [15] the new one). */
int prg_fr_mstep_from_arrays(int device, void* hip_stream, const double* t_source_hd, int64_t m, int dim,
                             int64_t n_target, const float* m0_hd, const float* m1_hd, const float* m2_hd,
                             const float* nx_hd, const double* rot9, const double* t3, double sigma2, double w,
                             double* out_host);

/* ---- Deformable kinematic FilterReg (dual-quaternion skinning) --------------------------------
 * A dual quaternion is 8 doubles (r_w, r_x, r_y, r_z, d_w, d_x, d_y, d_z); a point is tied to two nodes (`pairs`
 * [m x 2] int32) with two weights ([m x 2] float32, widened to fp64 on upload) and moves by their linear blend divided
 * by |r| (no antipodal sign correction).  All sums are fp64 with a fixed order, per "segment" = run of one ordered node
 * pair (pair0 * k_nodes + pair1, ascending); the 6K x 6K assembly and the minimum-norm solve are the caller's.
 *
 * prg_dq_skin: out[i] = blend(i).transform_point(points[i]), [m x 3] float64, no handle.
 * Replaces: DeformableKinematicModel.__init__ / _transform, transformation.py:209-212 (dq3d op.dlb, transform_point). */
int prg_dq_skin(int device, void* hip_stream, const double* points_hd, int64_t m, const int* pairs_hd,
                const float* weights_hd, const double* dualquats_hd, int k_nodes, double* out_hd);
/* Skinning weights of the plan's source (set the source first; a new source drops them).  Sorts the points by ordered
 * pair key once; *n_segments = number of distinct ordered pairs.  PRG_ERR_INVALID on an index outside [0, k_nodes) or a
 * wrong m - an earlier skinning then stays in place.  The dual quaternions start at the identity.
 * Replaces: DeformableKinematicFilterReg.__init__ filterreg.py:200-208, SkinningWeight.pairs_set / in_pair
 * transformation.py:187-194. */
int prg_fr_set_skinning(prg_filterreg* h, const int* pairs_hd, const float* weights_hd, int64_t m, int k_nodes,
                        int* n_segments);
/* The model's dual quaternions [k_nodes x 8], host memory.  Replaces: trans_p.dualquats, filterreg.py:206-208, 261. */
int prg_fr_set_dualquats(prg_filterreg* h, const double* dualquats_host, int k_nodes);
int prg_fr_get_dualquats(prg_filterreg* h, double* dualquats_host, int k_nodes);
/* Skin the stored source with the plan's dual quaternions on the device and run the lattice E-step of prg_fr_estep
 * over [skinned source; target] / sqrt(sigma2); m0, m1, m2 stay on the device (prg_fr_get_estep reads them).
 * Replaces: `self._tf_result.transform(self._source)` + expectation_step, filterreg.py:130-134, 78-100. */
int prg_fr_kinematic_estep(prg_filterreg* h, double sigma2, double alpha, int* lattice_size, int* with_blur);
/* E-step values from the caller instead of the plan's last E-step (m2 may be NULL), for the M-step on explicit arrays:
 * t_source [m x 3] float64, m0 [m], m1 [m x 3], m2 [m] float32, m = the plan's source size.  Holds until the next
 * prg_fr_kinematic_estep.  Replaces: the arguments of _maximization_step, filterreg.py:211-220. */
int prg_fr_kinematic_set_arrays(prg_filterreg* h, const double* t_source_hd, const float* m0_hd, const float* m1_hd,
                                const float* m2_hd, int64_t n_target);
/* Normal-matrix sums, once per M-step.  out_host [n_segments x 34] per segment: with s^2 = m0/(m0+c)/sigma2,
 * c = w/(1-w) n/m, and x the moved source: [0..9] sum w0^2 s^2 (1, x, y, z, xx, xy, xz, yy, yz, zz), [10..19] the same
 * under w0 w1, [20..29] under w1^2 (J^T J of J = [-[x]x | I] is linear in these), [30] numerator and [31] sum m0/(m0+c)
 * of the sigma2 update, [32] points that took part.  A point with m0 == 0 takes no part; reference_form != 0 gives it
 * m0 = float32 eps instead (filterreg.py:223).  Replaces: filterreg.py:222-236, 263-264. */
int prg_fr_kinematic_normal_sums(prg_filterreg* h, double sigma2, double w, int reference_form, int n_segments,
                                 double* out_host);
/* Gradient sums, once per inner iteration: twists_host [k_nodes x 6] are the current increments; every point is
 * skinned with dualquat_from_twist of them, rx = s (x - m1/m0).  out_host [n_segments x 16]: [0..5] sum w0 s J^T rx,
 * [6..11] sum w1 s J^T rx, [12] sum (rx_0 + rx_1 + rx_2)^2 (= np.dot(rx.T, rx).sum(), :265).  reference_form != 0
 * leaves a point whose two nodes coincide at x = 0, as the reference's loop over permutations does.
 * Replaces: filterreg.py:38-42, 238-254, 265. */
int prg_fr_kinematic_grad_sums(prg_filterreg* h, const double* twists_host, int reference_form, int n_segments,
                               double* out_host);
/* Both sums in one call on explicit arrays, no handle (twists_host NULL = zero increments); n_segments must be the
 * number of distinct ordered pairs.  Replaces: as the two calls above. */
int prg_fr_kinematic_sums_from_arrays(int device, void* hip_stream, const double* t_source_hd, int64_t m,
                                      int64_t n_target, const float* m0_hd, const float* m1_hd, const float* m2_hd,
                                      const int* pairs_hd, const float* weights_hd, int k_nodes, double sigma2, double w,
                                      int reference_form, const double* twists_host, int n_segments,
                                      double* normal_out_host, double* grad_out_host);

/* Weighted Kabsch on float32 clouds: centroids weighted by w, covariance by w^2; rot_host dim x dim
 * row-major, t_host dim.  Replaces: _kabsch.kabsch / kabsch2d (cc/kabsch_py.cc, cc/kabsch.cc:6-109). */
int prg_kabsch_weighted(int device, void* hip_stream, const float* model_hd, const float* target_hd,
                        const float* weight_hd, int64_t n, int dim, double* rot_host, double* t_host);

/* ---- GMMTree (hierarchical 8-ary GMM, probreg/gmmtree.py + cc/gmmtree.{h,cc}) ------------------------------------
 * Everything in fp64 (the reference's native code is float).  Node records are 10 doubles:
 *   pi, mu (3), Sigma (xx, xy, xz, yy, yz, zz); node j of level l sits at 8 (8^l - 1) / 7 + local index, the
 *   children of j at (j + 1) 8 ... + 7 (gmmtree.cc:42-44).  1 <= tree_level <= 4.  Results are reproducible: every
 *   sum over points is reduced in a fixed order (no floating-point atomics). */
typedef struct prg_gmmtree prg_gmmtree;
/* The pybind module probreg._gmmtree (cc/gmmtree_py.cc) as a handle: one device, one stream. */
int prg_gmm_create(prg_gmmtree** out, int device, void* hip_stream);
int prg_gmm_destroy(prg_gmmtree* h);
/* buildGmmTree (gmmtree.cc:98-123) with initializeNodes (:46-73) on explicit leaf indices init_idx_host[8^tree_level]
 * (the reference draws them from std::rand): points n x 3 float64.  Each level runs EM (gmmTreeEstep :125-163,
 * gmmTreeMstep :165-173, logLikelihood :20-33) until |q - q_prev| < lambda_s or max_iter iterations.  Out per level
 * (tree_level entries): iters_host, q_host (last q, may be NULL), dq_host (last |q - q_prev|, may be NULL). */
int prg_gmm_build(prg_gmmtree* h, const double* points_hd, int64_t n, int tree_level, const int64_t* init_idx_host,
                  double lambda_s, double lambda_d, int max_iter, int* iters_host, double* q_host, double* dq_host);
/* Install a given tree (n_nodes x 10 doubles, host) instead of building one; get_nodes reads the current tree back. */
int prg_gmm_set_nodes(prg_gmmtree* h, const double* nodes_host, int tree_level);
int prg_gmm_get_nodes(prg_gmmtree* h, double* nodes_host);
/* Target of the registration E-step: n x 3 float64, kept on the device across iterations. */
int prg_gmm_set_target(prg_gmmtree* h, const double* target_hd, int64_t n);
/* gmmTreeRegEstep (gmmtree.cc:175-214) on the target transformed by scale * rot9 (row-major) + t3
 * (GMMTree.registration gmmtree.py:87): per node m01_host[n_nodes x 4] = (m0, m1) and, if m2_host is not NULL,
 * m2_host[n_nodes x 6] = m2 (xx, xy, xz, yy, yz, zz).  Synchronises. */
int prg_gmm_reg_estep(prg_gmmtree* h, const double* rot9, const double* t3, double scale, double lambda_c,
                      double* m01_host, double* m2_host);

/* ---- Spherical Gaussian-mixture fit (the feature generator of GMMReg, probreg/features.py:54-69) ------------------
 * features.GMM.compute calls scikit-learn's GaussianMixture(n_components, covariance_type = "spherical").fit; these
 * entry points restate that fit in fp64 on the device.  Results are reproducible: every sum over points is reduced
 * in a fixed order (no floating-point atomics).  Means are k x dim, weights / covariances / precisions k doubles. */
typedef struct prg_gmmfit prg_gmmfit;
/* One fit context on one device / stream (features.GMM.init, features.py:64-65, creates the sklearn estimator). */
int prg_gmmfit_create(prg_gmmfit** out, int device, void* hip_stream);
int prg_gmmfit_destroy(prg_gmmfit* h);
/* The cloud of `self._clf.fit(data)` (features.py:68): n x dim float64, dim 2 or 3, uploaded once. */
int prg_gmmfit_set_data(prg_gmmfit* h, const double* data_hd, int64_t n, int dim);
/* Greedy k-means++ seeding of k centres (what sklearn's KMeans does first inside the fit's default init_params =
 * "kmeans"): uniforms_host[k x n_trials] in [0, 1), entry 0 draws the first centre, row s the n_trials <= 16
 * candidates of centre s by D^2 sampling; the candidate with the lowest potential is kept.  k <= n. */
int prg_gmmfit_seed(prg_gmmfit* h, int k, const double* uniforms_host, int n_trials);
/* Indices of the points the k seeds were taken from. */
int prg_gmmfit_get_seeds(prg_gmmfit* h, int* index_host);
/* Lloyd iterations from the seeds (sklearn KMeans: stop when no label changes or the summed squared centre shift is
 * <= tol, at most max_iter); an empty cluster keeps its centre.  n_iter_host may be NULL. */
int prg_gmmfit_lloyd(prg_gmmfit* h, int max_iter, double tol, int* n_iter_host);
/* The parameters sklearn's fit starts from: its M-step on the one-hot responsibilities of the Lloyd labels, with
 * weights = nk / n (BaseMixture._initialize_parameters -> GaussianMixture._initialize). */
int prg_gmmfit_init_from_labels(prg_gmmfit* h, double reg_covar);
/* Explicit start (sklearn's weights_init, means_init, precisions_init): precisions > 0, weights >= 0. */
int prg_gmmfit_set_params(prg_gmmfit* h, int k, const double* weights_host, const double* means_host,
                          const double* precisions_host);
/* EM from the current parameters (the loop of BaseMixture.fit_predict): E-step, M-step, lower bound = mean per-point
 * normaliser; stops when |change of the lower bound| < tol or after max_iter iterations.  lower_bounds_host (max_iter
 * doubles, may be NULL) receives the lower bound of every iteration run. */
int prg_gmmfit_em(prg_gmmfit* h, double tol, int max_iter, double reg_covar, int* n_iter_host, int* converged_host,
                  double* lower_bounds_host);
/* means_ / weights_ / covariances_ (features.py:69 returns the first two); each pointer may be NULL.  After seed or
 * lloyd only the centres (means) exist. */
int prg_gmmfit_get_params(prg_gmmfit* h, double* weights_host, double* means_host, double* covariances_host);

/* ---- One-class nu-SVM with the RBF kernel (the feature generator of SVR, probreg/features.py:72-100) ---------------
 * features.OneClassSVM.compute calls scikit-learn's svm.OneClassSVM(nu, kernel = "rbf", gamma).fit (libsvm); these
 * entry points solve the same dual in fp64 on the device, in libsvm's scaling: minimise 1/2 a'Qa subject to
 * 0 <= a_i <= 1 and sum a_i = nu n, with Q_ij = exp(-gamma |x_i - x_j|^2).  Working-set decomposition (csrc/ocsvm.hip);
 * two solves of the same input give byte-identical results (fixed-order reductions, no floating-point atomics). */
typedef struct prg_ocsvm prg_ocsvm;
/* One solver context on one device / stream (features.OneClassSVM.init, features.py:91-92, creates the estimator). */
int prg_ocsvm_create(prg_ocsvm** out, int device, void* hip_stream);
int prg_ocsvm_destroy(prg_ocsvm* h);
/* Points per working set (no counterpart in scikit-learn: libsvm works on pairs).  Needs no device. */
int prg_ocsvm_working_set_size(int* q_host);
/* The cloud of `self._clf.fit(data)` (features.py:95): n x dim float64, dim 2 or 3, finite, uploaded once. */
int prg_ocsvm_set_data(prg_ocsvm* h, const double* data_hd, int64_t n, int dim);
/* The fit itself (libsvm solve_one_class / Solver::Solve): from libsvm's start (the first floor(nu n) points at the
 * bound), rounds of working-set selection, second-order SMO on the set (at most inner_cap steps) and gradient update,
 * until the maximal KKT violation m - M < tol (scikit-learn's `tol`, default 1e-3) or max_iter rounds are done
 * (scikit-learn's `max_iter` counts single SMO steps instead).  gamma > 0, 0 < nu <= 1.  n_iter_host: rounds that
 * changed a; n_inner_host (may be NULL): SMO steps of all rounds; converged_host: 0 when max_iter ended the loop (the
 * solution is feasible all the same, as with libsvm's warning); gap_host: m - M of the returned solution (-inf when
 * every a is at the upper bound). */
int prg_ocsvm_solve(prg_ocsvm* h, double gamma, double nu, double tol, int max_iter, int inner_cap, int* n_iter_host,
                    int* n_inner_host, int* converged_host, double* gap_host);
/* The solution: alpha_host[n] (dense; scikit-learn's dual_coef_ is its non-zero part), rho (scikit-learn's offset_),
 * the objective 1/2 a'Qa and the number of support vectors; each pointer may be NULL. */
int prg_ocsvm_get_solution(prg_ocsvm* h, double* alpha_host, double* rho_host, double* objective_host,
                           int* n_support_host);
/* scikit-learn's support_: the indices with a_i > 0, ascending. */
int prg_ocsvm_get_support(prg_ocsvm* h, int* index_host);
/* sum_i a_i exp(-gamma |x_i - p|^2) at k points (k x dim float64, host or device) with the gamma of the last solve:
 * scikit-learn's score_samples; decision_function is this minus rho.  Synchronises. */
int prg_ocsvm_decision(prg_ocsvm* h, const double* points_hd, int64_t k, double* out_hd);
/* Timing split for tools (no counterpart): with profile on, a solve records device milliseconds of
 * ms4_host = (initial gradient, selection, subproblem, gradient sweep) summed over its rounds. */
int prg_ocsvm_set_profile(prg_ocsvm* h, int on);
int prg_ocsvm_get_profile(prg_ocsvm* h, double* ms4_host);

/* ---- FPFH descriptor (probreg/features.py:28-51, which calls Open3D) ---------------------------------------------
 * features.FPFH.compute calls Open3D's estimate_normals(KDTreeSearchParamHybrid) and compute_fpfh_feature; these entry
 * points restate both in fp64 on the device, one stage per call (csrc/fpfh.hip; the definition with every tie rule is
 * DESIGN.md section 3.9).  Two runs on the same input give byte-identical results (no floating-point atomics). */
typedef struct prg_fpfh prg_fpfh;
/* One descriptor context on one device / stream (features.FPFH.__init__, features.py:36-38, builds the search parameters). */
int prg_fpfh_create(prg_fpfh** out, int device, void* hip_stream);
int prg_fpfh_destroy(prg_fpfh* h);
/* Longest neighbour list a search can return (no counterpart: Open3D's max_nn is unbounded).  Needs no device. */
int prg_fpfh_max_nn(int* max_nn_host);
/* The cloud `pcd.points` (features.py:47-48): n x 3 float64, finite, host or device, uploaded once. */
int prg_fpfh_set_data(prg_fpfh* h, const double* points_hd, int64_t n);
/* Open3D's KDTreeSearchParamHybrid(radius, max_nn) for every point: which = 0 keeps the lists of the normals
 * (features.py:37), which = 1 those of the histograms (features.py:38).  A list is the point itself, then the other
 * points with d2 <= radius^2 by ascending (d2, index), cut to max_nn entries; 1 <= max_nn <= prg_fpfh_max_nn. */
int prg_fpfh_search(prg_fpfh* h, int which, double radius, int max_nn);
/* The lists of a search: idx_host / d2_host are n x max_nn (unused entries -1 / 0), count_host n; each may be NULL. */
int prg_fpfh_get_neighbours(prg_fpfh* h, int which, int* idx_host, double* d2_host, int* count_host);
/* estimate_normals (features.py:43-44) on the lists of search 0: unit eigenvector of the smallest eigenvalue of the
 * population covariance of the listed points, largest component positive; (0, 0, 1) for fewer than 3 entries. */
int prg_fpfh_normals(prg_fpfh* h);
/* Caller-supplied normals instead (a cloud that arrives with normals): n x 3 float64, host or device. */
int prg_fpfh_set_normals(prg_fpfh* h, const double* normals_hd);
int prg_fpfh_get_normals(prg_fpfh* h, double* normals_host);
/* The simplified point feature histograms over the lists of search 1 (first half of compute_fpfh_feature, features.py:50):
 * n x 33, every 11-bin group of a row with neighbours sums to 100. */
int prg_fpfh_spfh(prg_fpfh* h);
int prg_fpfh_get_spfh(prg_fpfh* h, double* spfh_host);
/* The descriptor (second half of compute_fpfh_feature): the neighbours' SPFH rows weighted by 1 / d2, every group scaled
 * to sum 100, plus the point's own SPFH row; n x 33 (Open3D's `.data` is the transpose, features.py:51 transposes back). */
int prg_fpfh_fpfh(prg_fpfh* h);
int prg_fpfh_get_fpfh(prg_fpfh* h, double* fpfh_host);

/* ---- Global registration: feature matching and RANSAC pose search ----------------------------------------------------
 * None of this is in the reference: its examples get a start pose from Open3D (compute_fpfh_feature, then
 * registration_ransac_based_on_feature_matching).  These entry points restate that pipeline in fp64 on the device
 * (csrc/global_reg.hip; the definition with every order of summation and every tie rule is DESIGN.md section 3.13).
 * Two runs on the same input give byte-identical results (no floating-point atomics). */
/* For every row of a (na x d float64, host or device) the row of b (nb x d) of least squared distance, accumulated over the
 * d columns in ascending order with every operation rounded once; ties go to the smaller index.  1 <= d <= 64.  segments:
 * pieces the streamed side is cut into (0: automatic; the result does not depend on it).  idx_out_hd na int32, d2_out_hd na
 * float64.  Replaces: none in the reference; the correspondence search inside Open3D's
 * registration_ransac_based_on_feature_matching in its examples.  Synchronises. */
int prg_feature_match(int device, void* hip_stream, const double* a_hd, int64_t na, const double* b_hd, int64_t nb, int d,
                      int segments, int* idx_out_hd, double* d2_out_hd);
/* The same plus the sweep with the roles swapped: mutual_out_hd[a] = 1 iff a is also the best row of a for idx[a]
 * (Open3D's mutual_filter).  Replaces: none in the reference (see prg_feature_match). */
int prg_feature_match_mutual(int device, void* hip_stream, const double* a_hd, int64_t na, const double* b_hd, int64_t nb,
                             int d, int segments, int* idx_out_hd, double* d2_out_hd, int* mutual_out_hd);
typedef struct prg_ransac prg_ransac;
/* One pose search on one device / stream.  Replaces: none in the reference; Open3D's
 * registration_ransac_based_on_feature_matching in its examples (as every prg_ransac_* entry point below). */
int prg_ransac_create(prg_ransac** out, int device, void* hip_stream);
int prg_ransac_destroy(prg_ransac* h);
/* The correspondences: source points p_hd and matched target points q_hd, C x 3 float64 each (host or device), C >= 3. */
int prg_ransac_set_correspondences(prg_ransac* h, const double* p_hd, const double* q_hd, int64_t C);
/* Hypotheses h_offset .. h_offset + H - 1 of the stream `seed`: hypothesis h draws three correspondences by splitmix64 on the
 * counters 3h + 1 .. 3h + 3, is valid iff the indices are distinct, every edge passes Open3D's edge-length check with
 * edge_similarity in [0, 1] and the source triangle is not degenerate, and then gets the Kabsch pose of its three pairs.
 * Invalid draws are not redrawn.  Two calls that cover a range in pieces give what one call gives. */
int prg_ransac_build(prg_ransac* h, uint64_t seed, uint64_t h_offset, int64_t H, double edge_similarity);
/* The hypotheses: triples_host H x 3 int32 (built hypotheses only), pose_host H x 12 (rotation row-major, then the shift;
 * zeros where invalid), valid_host H int32; each may be NULL. */
int prg_ransac_get_hypotheses(prg_ransac* h, int* triples_host, double* pose_host, int* valid_host);
/* Install explicit hypotheses instead of building them (the scoring stage on its own). */
int prg_ransac_set_hypotheses(prg_ransac* h, const double* pose_host, const int* valid_host, int64_t H);
/* Per valid hypothesis: the number of correspondences with |R p + t - q|^2 <= tau^2 and the sum of those squares in
 * ascending order (segments of 1024 correspondences, segment sums added in ascending order).  The sweep runs over the valid hypotheses only (their indices are compacted
 * first); waits for their number, then enqueues. */
int prg_ransac_score(prg_ransac* h, double tau);
/* counts_host H int32 (-1 for an invalid hypothesis), sums_host H float64 (0 there); each may be NULL. */
int prg_ransac_get_scores(prg_ransac* h, int* counts_host, double* sums_host);
/* The winner: largest count, then smallest sum, then smallest index; each pointer may be NULL.  PRG_ERR_STATE with a message
 * when no hypothesis is valid. */
int prg_ransac_best(prg_ransac* h, int64_t* index_host, int* count_host, double* sum_host, double* pose_host);
/* `iters` refits from pose_io_host (12 doubles, overwritten with the result): Kabsch over the inliers of the current pose,
 * sums in ascending order (runs of 64 correspondences, run sums added in ascending order); a pose with fewer than 3 inliers
 * is kept.  Then count_host / sum_host / inlier_host (C int32 flags) at the final pose; each may be NULL.  Synchronises. */
int prg_ransac_refine(prg_ransac* h, double tau, int iters, double* pose_io_host, int* count_host, double* sum_host,
                      int* inlier_host);

/* ---- Voxel down-sampling ------------------------------------------------------------------------------------------------
 * None of this is in the reference: every 3-D example of it calls Open3D's voxel_down_sample(voxel_size) on both clouds
 * before it registers (examples/utils.py: prepare_source_and_target_rigid_3d, prepare_source_and_target_nonrigid_3d).  These
 * entry points restate PointCloud::VoxelDownSample in fp64 on the device (csrc/voxel.hip; the definition with the order of
 * the voxels and of every sum is DESIGN.md section 3.14).  Two runs on the same input give byte-identical results (no
 * floating-point atomics), whatever the launch geometry. */
typedef struct prg_voxel prg_voxel;
/* One down-sampling context on one device / stream; a plan can be run again with other data or another voxel size.
 * Replaces: none in the reference; Open3D's voxel_down_sample in its examples (as every prg_voxel_* entry point below). */
int prg_voxel_create(prg_voxel** out, int device, void* hip_stream);
int prg_voxel_destroy(prg_voxel* h);
/* The cloud (`pcd.points` of the examples): n x d float64, d = 2 or 3, finite, host or device, 1 <= n < 2^31; uploaded once.
 * Drops the channels of an earlier cloud. */
int prg_voxel_set_data(prg_voxel* h, const double* points_hd, int64_t n, int d);
/* Per-point channels that are averaged like the coordinates (Open3D averages `pcd.normals` and `pcd.colors`): n x c float64,
 * 0 <= c <= 67 - the caller puts normals and attributes side by side; c = 0 removes them. */
int prg_voxel_set_channels(prg_voxel* h, const double* channels_hd, int c);
/* voxel_down_sample(v): cells floor((p - (min - v / 2)) / v) per axis, voxels in ascending (c_x, c_y, c_z), the points of a
 * voxel in ascending index, sums over pieces of 64 sorted positions (section 3.14).  v > 0 and finite.  PRG_ERR_INVALID,
 * before anything is sorted, when an axis needs 2^21 cells or more (Open3D allows INT_MAX).  Waits twice (the box, the
 * number of voxels). */
int prg_voxel_run(prg_voxel* h, double v);
/* The number of voxels V of the last run (len(result.points) in Open3D). */
int prg_voxel_count(prg_voxel* h, int64_t* v_host);
/* Open3D's result.points: V x d means.  And result.normals / result.colors: V x c channel means, not renormalised. */
int prg_voxel_get_means(prg_voxel* h, double* means_host);
int prg_voxel_get_channel_means(prg_voxel* h, double* means_host);
/* Per voxel: the number of its points and the smallest original index among them, V int32 each (no counterpart in
 * voxel_down_sample; Open3D's voxel_down_sample_and_trace reports the members). */
int prg_voxel_get_counts(prg_voxel* h, int* counts_host);
int prg_voxel_get_first(prg_voxel* h, int* first_host);
/* Per input point the row of its voxel, n int32 (the first result of voxel_down_sample_and_trace, inverted). */
int prg_voxel_get_inverse(prg_voxel* h, int* inverse_host);
/* The stages of the last run, for tests and tools (no counterpart: Open3D keeps a hash map): the key c_x 2^42 + c_y 2^21 +
 * c_z of every point (n uint64), the point at every position of the stably sorted sequence (n int32), and the voxel row of
 * every sorted position (n int32). */
int prg_voxel_get_keys(prg_voxel* h, uint64_t* keys_host);
int prg_voxel_get_order(prg_voxel* h, int* order_host);
int prg_voxel_get_rows(prg_voxel* h, int* rows_host);

/* ---- ICP: point-to-point and point-to-plane on a grid nearest-neighbour search ----------------------------------------------
 * None of this is in the reference: examples/time_measurement.py and examples/icp_test.py call Open3D's registration_icp.
 * These entry points restate it in fp64 on the device (csrc/icp.hip, the search in csrc/grid_search.hip; the definition with the tie rule of the search, the
 * order of every sum and the loop is DESIGN.md section 3.15).  Two runs on the same input give byte-identical results (no
 * floating-point atomics), whatever the launch geometry and the grid.  kind: 0 point-to-point, 1 point-to-plane, 2 generalized
 * (needs covariances, see the end of this section). */
typedef struct prg_icp prg_icp;
/* One ICP context on one device / stream; the pose starts as the identity.  Replaces: none in the reference; Open3D's
 * registration_icp / evaluate_registration in its examples (as every prg_icp_* entry point below). */
int prg_icp_create(prg_icp** out, int device, void* hip_stream);
int prg_icp_destroy(prg_icp* h);
/* The target: n x 3 float64, finite, host or device, 1 <= n < 2^31, and its normals (n x 3, or NULL: point-to-point only).
 * Builds the search grid once (and coarser levels of it, for queries far from the cloud); cell_edge > 0 sets the finest cell
 * edge, 0 lets the cloud choose it (a few distinct points per occupied cell); either is raised to the largest extent / 2^30, so
 * that the levels always reach one on which the box is two cells wide.  The grid never changes a result.  Memory: about
 * 64 n bytes plus 32 to 48 n bytes per level.  Synchronises. */
int prg_icp_set_target(prg_icp* h, const double* points_hd, const double* normals_hd, int64_t n, double cell_edge);
/* The finest grid of the target: its cell edge, cells per axis (3 int32), whether the cells are addressed directly (1) or
 * hashed (0), and the number of levels (each four times coarser than the one below); each may be NULL.  For tools (no
 * counterpart). */
int prg_icp_get_grid(prg_icp* h, double* cell_edge_host, int* dims_host, int* dense_host, int* levels_host);
/* The source: m x 3 float64, finite, host or device, 1 <= m < 2^31.  Synchronises. */
int prg_icp_set_source(prg_icp* h, const double* points_hd, int64_t m);
/* The pose q = R p + t as 12 doubles: R row-major, then t (registration_icp's `init`). */
int prg_icp_set_pose(prg_icp* h, const double* pose_host);
int prg_icp_get_pose(prg_icp* h, double* pose_host);
/* For every moved source point the target index of the smallest (d2, index) among d2 <= r * r, -1 when there is none;
 * r > 0, infinity allowed.  Enqueues only. */
int prg_icp_search(prg_icp* h, double r);
/* The matches of the last search: index_host m int32, d2_host m float64 (+inf where unmatched); each may be NULL. */
int prg_icp_get_matches(prg_icp* h, int* index_host, double* d2_host);
/* The raw ordered sums of a step over the current matches, out_host 32 doubles (unused ones 0): kind 0: count, sum d2,
 * sum q (3), sum y (3), then the centred products (q - qm)_a (y - ym)_b (9, a major); kind 1: count, sum d2, the upper
 * triangle of sum J J^T (21, row-major), sum J res (6).  Synchronises. */
int prg_icp_sums(prg_icp* h, int kind, double* out_host);
/* One step on the current matches: Kabsch (kind 0, at least 3 matches) or the 6 x 6 Cholesky solve (kind 1, at least 6 matches
 * and no pivot <= 1e-12 max diag).  A missing step leaves the pose as it is and shows in the status.  Enqueues only. */
int prg_icp_step(prg_icp* h, int kind);
/* Open3D's loop from the current pose: evaluate, then up to max_iteration times step and evaluate; stops converged when
 * fitness and rmse both change by less than rel_fitness / rel_rmse, and unconverged on a missing step.  The stop test runs
 * on the device; the host looks at the flag every `chunk` iterations, and the result does not depend on chunk. */
int prg_icp_iterate(prg_icp* h, int kind, double r, int max_iteration, double rel_fitness, double rel_rmse, int chunk);
/* After prg_icp_iterate (or a single stage): pose_host 12 doubles, the matched count and the ordered sum of d2 of the last
 * evaluation, the steps done, converged (0 / 1) and the status: 0 ok, 1 fewer than 3 matches (kind 0), 2 degenerate (kind 1:
 * fewer than 6 matches or a pivot at the floor).  Each may be NULL.  Synchronises. */
int prg_icp_get_state(prg_icp* h, double* pose_host, int64_t* count_host, double* sum_host, int* n_iter_host,
                      int* converged_host, int* status_host);
/* ---- Generalized ICP (plane-to-plane; Segal et al., Open3D's registration_generalized_icp): kind 2 of prg_icp_sums,
 * prg_icp_step and prg_icp_iterate, on the same search, ordered sums, Cholesky step and loop.  Every
 * point of both clouds carries a symmetric positive-definite 3 x 3 covariance, 6 doubles (xx, xy, xz, yy, yz, zz); a matched
 * pair is weighted by the inverse of C_target + R C_source R^T.  prg_icp_sums then gives: count, sum d2, the upper triangle of
 * sum J^T P J (21), sum J^T P d (6) and, in slot 29, the objective sum d^T P d.  Fitness, rmse and the stop test stay
 * Euclidean.  Kind 2 without both sets of covariances is PRG_ERR_STATE.  which: 0 source, 1 target; the cloud must be set, n
 * is its number of points, and setting the cloud again drops its covariances.  None of this is in the reference. */
/* Explicit covariances, n x 6 float64, host or device: finite, and positive definite by the pivot rule of the step (no
 * Cholesky pivot <= 1e-12 max diag).  Replaces: the `covariances` of the clouds handed to registration_generalized_icp.
 * Synchronises. */
int prg_icp_set_covariances(prg_icp* h, int which, const double* cov_hd, int64_t n);
/* Covariances I - (1 - epsilon) u u^T from normals (n x 3 float64, host or device, every norm finite and > 0; u = n / |n|),
 * 0 < epsilon <= 1: Open3D's R diag(epsilon, 1, 1) R^T in closed form, independent of the sign of the normal.  Computed on the
 * device.  Synchronises. */
int prg_icp_set_covariances_from_normals(prg_icp* h, int which, const double* normals_hd, int64_t n, double epsilon);
/* The covariances of a cloud as they are stored, n x 6 float64 to the host.  Synchronises. */
int prg_icp_get_covariances(prg_icp* h, int which, double* cov_host);
/* ---- Exact k-nearest-neighbour lists, radius counts and the two outlier filters on the same grid, levels and query order
 * (none of this is in the reference, whose examples leave cleaning a cloud to Open3D).  The queries
 * are the source points moved by the pose, the cloud is the target; fp64, no floating-point atomics, byte-identical from run
 * to run and independent of the grid.  Setting a cloud or the pose, a step and the loop drop the lists, counts and filter
 * results; new lists drop the result of the statistical filter and new counts that of the radius filter, whose keep masks
 * were made from the ones before. */
/* The largest k of prg_icp_knn and prg_icp_outlier_statistical (64: one list entry per lane of a wave). */
int prg_icp_max_k(int* out);
/* For every moved source point the targets with d2 <= r * r in ascending (d2, index), cut to k entries; 1 <= k <= 64, r > 0,
 * infinity allowed.  k = 1 is prg_icp_search.  A query that is itself a target point is an ordinary candidate with d2 = 0.
 * Replaces: a kd-tree's search_knn / search_hybrid.  Enqueues only. */
int prg_icp_knn(prg_icp* h, int k, double r);
/* The lists of the last prg_icp_knn (or prg_icp_outlier_statistical): index_host m x k int32 and d2_host m x k float64, the
 * slots past a list's length -1 and +inf; count_host m int32, the lengths.  Each may be NULL.  Synchronises. */
int prg_icp_get_knn(prg_icp* h, int* index_host, double* d2_host, int* count_host);
/* For every moved source point the number of targets with d2 <= r * r; r finite and > 0.  Replaces: the length of a kd-tree's
 * search_radius.  Enqueues only. */
int prg_icp_radius_count(prg_icp* h, double r);
/* The counts of the last prg_icp_radius_count (or prg_icp_outlier_radius), m int32.  Synchronises. */
int prg_icp_get_counts(prg_icp* h, int* count_host);
/* Open3D's remove_statistical_outlier on the source, which the caller has also set as the target: the lists of k = nb_neighbors
 * with r = infinity (the point itself is one of them), a_i the mean of their distances, mu and s the mean and the sample
 * standard deviation of the a_i in runs of 64, thr = mu + std_ratio * s; point i is kept iff a_i <= thr (Open3D: <, and a_i > 0).
 * std_ratio finite and >= 0.  Enqueues only. */
int prg_icp_outlier_statistical(prg_icp* h, int k, double std_ratio);
/* Open3D's remove_radius_outlier, source and target set alike: point i is kept iff its radius count, itself included, is
 * > nb_points; r finite and > 0, nb_points >= 0.  Enqueues only. */
int prg_icp_outlier_radius(prg_icp* h, double r, int nb_points);
/* The last filter: keep_host m bytes (1 kept, 0 removed); after the statistical filter also score_host m float64 (a_i) and
 * stat_host 3 float64 (mu, s, thr), which must be NULL after the radius filter (its scores are prg_icp_get_counts).  Each may
 * be NULL.  Synchronises. */
int prg_icp_get_outlier(prg_icp* h, unsigned char* keep_host, double* score_host, double* stat_host);
/* DBSCAN of the source, which the caller has also set as the target, at the identity pose (csrc/icp_cluster.hip):
 * c_i the radius count of eps, the point itself included; point i is core iff c_i >= min_points; the clusters are the connected
 * components of the core points under d2 <= eps * eps, numbered 0, 1, ... in ascending order of their smallest core index; a
 * point that is not core takes the cluster of its nearest core neighbour within eps, the minimum of (d2, index) (Open3D and
 * scikit-learn: the cluster that reaches it first), or -1, noise, when it has none.  eps finite and > 0, min_points >= 1, as many
 * target as source points.  Integer atomics only; independent of the grid, the launch geometry and the run.  Replaces: none in the
 * reference; Open3D's cluster_dbscan(eps, min_points).  Enqueues only. */
int prg_icp_dbscan(prg_icp* h, double eps, int min_points);
/* The last prg_icp_dbscan: labels_host m int32 (-1: noise), core_host m bytes (1 core, 0 not), n_clusters_host one int32 and
 * sizes_host n_clusters int32, the members of every cluster with its border points (its length is known from a first call with
 * sizes_host NULL).  Each may be NULL.  The counts c_i are prg_icp_get_counts.  Synchronises. */
int prg_icp_get_dbscan(prg_icp* h, int* labels_host, unsigned char* core_host, int* n_clusters_host, int* sizes_host);

/* ---- Kernel fields: a non-rigid result evaluated at any points ------------------------------------------------------------
 * f(x)_c = sum_m k(|x - y_m|^2) w_mc over M control points y_m (D = 2 or 3) with C <= 4 weight columns, for Q query points x
 * that need not be the control points: the displacement field behind NonRigidTransformation (gaussian), CombinedTransformation
 * (imq) and TPSTransformation (tps), which the reference only ever evaluates through an M x M or Q x K float32 kernel matrix.
 * fp64 throughout (differences, d2, kernel, sums), straight from the caller's coordinates; control points in ascending index
 * in slabs of 65 536 whose sums are added in ascending order, no floating-point atomics: byte-identical from run to run and
 * independent of Q, of the launch geometry and of the batching of the queries (csrc/field.hip). */
#define PRG_FIELD_GAUSSIAN 0 /* exp(-d2 / (2 param)), param = beta > 0: math_utils.rbf_kernel (2 beta, not 2 beta^2) */
#define PRG_FIELD_IMQ 1      /* 1 / sqrt(d2 + param), param = c > 0: math_utils.inverse_multiquadric_kernel */
#define PRG_FIELD_TPS 2      /* math_utils.tps_kernel: D = 2: d2 log(d2) / 2 where d2 > 1e-9, else 0; D = 3: -sqrt(d2) */
typedef struct prg_field prg_field;
/* One field on one device / stream; the control points can be set again.  Replaces: none in the reference (as every
 * prg_field_* entry point below); the nearest is `np.dot(kernel(points, control), weights)` of transformation.py:81-160. */
int prg_field_create(prg_field** out, int device, void* hip_stream);
int prg_field_destroy(prg_field* h);
/* The control points (m x d float64) and their weights (m x c float64), finite, host or device, 1 <= m < 2^31, d = 2 or 3,
 * 1 <= c <= 4; kind and param as above (param is ignored for PRG_FIELD_TPS).  Packed once into [y, w] rows.  Synchronises. */
int prg_field_set_control(prg_field* h, const double* control_hd, const double* weights_hd, int64_t m, int d, int c, int kind,
                          double param);
/* f at q points (q x d float64, finite, host or device, 0 <= q < 2^31) -> out_host q x c float64.  With more than 65 536
 * control points the queries go through in batches that keep the slab sums within 64 MB.  Synchronises. */
int prg_field_evaluate(prg_field* h, const double* points_hd, int64_t q, double* out_host);

/* ---- plane segmentation (csrc/plane_seg.hip, csrc/plane_seg.h) ----
 * The dominant plane of a 3-D cloud by RANSAC: hypotheses x points in fp64, every operation rounded once, sums in a stated
 * order, no floating-point atomics; every stage can be driven on its own.  A plane is six doubles: the unit normal n (its
 * component of largest magnitude positive) and an anchor a; the signed distance of x is
 * (n_x (x - a_x) + n_y (y - a_y)) + n_z (z - a_z).  A point is an inlier iff |dist| <= tau and, with cos_theta >= 0 and normals
 * m, |n . m| >= cos_theta |m| with |m| > 0; a negative cos_theta switches the normal test off. */
typedef struct prg_plane prg_plane;
/* One segmentation on one device / stream.  Replaces: none in the reference (as every prg_plane_* entry point below); Open3D's
 * segment_plane(distance_threshold, ransac_n = 3, num_iterations), which users run on a scene before cluster_dbscan. */
int prg_plane_create(prg_plane** out, int device, void* hip_stream);
int prg_plane_destroy(prg_plane* h);
/* The cloud (n x 3 float64, finite, host or device, 3 <= n < 2^31) and, optionally (NULL: none), one normal per point (n x 3;
 * any length, its length is taken once here).  Synchronises. */
int prg_plane_set_points(prg_plane* h, const double* points_hd, const double* normals_hd, int64_t n);
/* The number of points of the handle's cloud: n, less what prg_plane_remove has dropped. */
int prg_plane_count(prg_plane* h, int64_t* n_host);
/* Hypotheses h_offset .. h_offset + H - 1 (1 <= H <= 2^24): point j of hypothesis g is splitmix64(seed, 3 g + j + 1) reduced to
 * [0, n); valid iff the three are distinct and |e1 x e2| >= 0.05 |e1| |e2|, > 0; the plane is n = (e1 x e2) / |e1 x e2| with the
 * sign rule, anchored at the first point. */
int prg_plane_build(prg_plane* h, uint64_t seed, uint64_t h_offset, int64_t H);
/* triples H x 3, planes H x 6 (zeros where invalid), valid H; any may be NULL.  Synchronises. */
int prg_plane_get_hypotheses(prg_plane* h, int* triples_host, double* planes_host, int* valid_host);
/* Installs H planes (H x 6) and their flags instead of drawing them (tests).  Synchronises. */
int prg_plane_set_hypotheses(prg_plane* h, const double* planes_hd, const int* valid_hd, int64_t H);
/* Per valid hypothesis the inlier count and the sum of dist^2 over the inliers: ascending index inside pieces of 1024 points,
 * the pieces added in ascending order.  An invalid hypothesis reports (-1, 0). */
int prg_plane_score(prg_plane* h, double tau, double cos_theta);
int prg_plane_get_scores(prg_plane* h, int* counts_host, double* sums_host);
/* The first hypothesis in the order (count descending, sum ascending, index ascending): its index (-1 when no hypothesis is
 * valid: count 0, sum 0, a plane of zeros), the number of valid hypotheses, count, sum and plane (6).  Any output may be NULL.
 * Synchronises. */
int prg_plane_best(prg_plane* h, int64_t* index_host, int64_t* n_valid_host, int* count_host, double* sum_host,
                   double* plane_host);
/* `iters` (0 .. 1000) least-squares refits of plane_io_host (6): over the inliers of the current plane, in runs of 64 points
 * added in ascending order, k = sum 1, s = sum q and sum q q^T (xx, xy, xz, yy, yz, zz) with q = x - a; c = s / k,
 * C = sum q q^T / k - c c^T; n = the eigenvector of C's smallest eigenvalue, a += c.  With fewer than three inliers the plane is
 * kept.  trace_host (iters x 10, may be NULL): the ten sums of every iteration.  Synchronises. */
int prg_plane_refine(prg_plane* h, double tau, double cos_theta, int iters, double* plane_io_host, double* trace_host);
/* Inlier mask (n, int) and signed distances (n) of plane_host (6), the inlier count and the sum of dist^2 in the order of
 * prg_plane_score.  Outputs may be NULL.  Synchronises. */
int prg_plane_classify(prg_plane* h, const double* plane_host, double tau, double cos_theta, int* mask_host, double* dist_host,
                       int* count_host, double* sum_host);
/* Drops the inliers of the last prg_plane_classify: the other points (and normals), in ascending index, become the handle's
 * cloud, which stays on the device; the hypotheses go.  n_left_host (may be NULL): the points left.  Synchronises. */
int prg_plane_remove(prg_plane* h, int64_t* n_left_host);

/* ---- fast global registration (csrc/fgr.hip, csrc/fgr.h) ----
 * Zhou, Park, Koltun (ECCV 2016), as Open3D's registration_fgr_based_on_correspondence runs it: one rigid pose (no scale) for
 * all correspondences by Gauss-Newton under a Geman-McClure line process whose scale mu is annealed, after a tuple test that
 * removes most wrong matches.  fp64, every operation rounded once, sums in runs of 64 rows added in ascending order, no
 * floating-point atomics; every stage can be driven on its own.  A pose is 12 doubles: the rotation row-major, then the shift. */
typedef struct prg_fgr prg_fgr;
/* One registration on one device / stream.  Replaces: none in the reference (as every prg_fgr_* entry point below); Open3D's
 * registration_fgr_based_on_correspondence, which users of the reference can get their start pose from. */
int prg_fgr_create(prg_fgr** out, int device, void* hip_stream);
int prg_fgr_destroy(prg_fgr* h);
/* Both clouds (m x 3 and n x 3 float64, finite, host or device, 1 <= m, n < 2^31).  Synchronises. */
int prg_fgr_set_clouds(prg_fgr* h, const double* source_hd, int64_t m, const double* target_hd, int64_t n);
/* c pairs (source index, target index), c x 2 int32, 3 <= c <= 2^31 / 100; the indices are checked by prg_fgr_normalise.
 * Synchronises. */
int prg_fgr_set_correspondences(prg_fgr* h, const int* corr_hd, int64_t c);
/* The mean of every cloud (all of its points: runs of 64 rows added in ascending order, the runs added in ascending order,
 * divided by the count), scale = the largest |x - mean| of both clouds, and the matched pairs as (x - mean) / scale_global with
 * scale_global = scale, or 1 with use_absolute_scale.  Outputs (3, 3, 1) may be NULL.  With a scale of 0 the pairs are not formed
 * and the later stages report PRG_ERR_STATE.  PRG_ERR_INVALID: a correspondence indexes outside its cloud.  Synchronises. */
int prg_fgr_normalise(prg_fgr* h, int use_absolute_scale, double* mean_p_host, double* mean_q_host, double* scale_host);
/* Trials per launch of prg_fgr_tuples (0: the default); bounds buffers, changes no result. */
int prg_fgr_set_chunk(prg_fgr* h, int64_t trials);
/* The tuple test: trial t = 0, 1, .. < 100 c draws three correspondences (splitmix64(seed, 3 t + j + 1) reduced to [0, c)) and
 * passes iff li s < lj and lj s < li on each of the edges (0, 1), (1, 2), (2, 0), li and lj the edge's lengths in the two
 * normalised clouds, s = tuple_scale in (0, 1].  The first maximum_tuple_count passing trials in ascending t are accepted; their
 * 3 indices each, in that order, become the used pairs.  n_trials: the last accepted trial + 1, or 100 c when the limit ended
 * the search.  Synchronises. */
int prg_fgr_tuples(prg_fgr* h, uint64_t seed, double tuple_scale, int64_t maximum_tuple_count, int64_t* n_tuples_host,
                   int64_t* n_trials_host);
/* Installs k >= 0 used pairs by their indices into the correspondences (k int32; repeats allowed).  PRG_ERR_INVALID: an index
 * outside [0, c).  Synchronises. */
int prg_fgr_set_used(prg_fgr* h, const int* index_hd, int64_t k);
/* The k indices of the used pairs.  Synchronises. */
int prg_fgr_get_used(prg_fgr* h, int* index_host);
/* Pose (of the normalised clouds) and mu > 0; clears the status and the step counter.  Synchronises. */
int prg_fgr_set_state(prg_fgr* h, const double* pose_host, double mu);
/* The 28 sums over the used pairs at the state's pose and mu: l J^T J (upper triangle, row-major, 21), l J^T r (6) and the
 * objective sum l r2 + mu (1 - sqrt l)^2, with s = R p + t, r = s - q, l = (mu / (mu + r2))^2, J = (-[s]x | I); runs of 64
 * pairs in ascending order, the runs added in ascending order.  sums_host (28) may be NULL.  Synchronises. */
int prg_fgr_sums(prg_fgr* h, double* sums_host);
/* One step from the sums: x = -A^-1 g by Cholesky (a pivot <= 1e-12 max diag A: degenerate), T <- dT(x) T with Open3D's
 * TransformVector6dToMatrix4d; then, with decrease_mu, after step i = 0, 4, 8, .. and while mu > maximum_correspondence_distance,
 * mu <- mu / division_factor.  Fewer than three used pairs or a failed pivot set the status, stop the loop and leave the pose. */
int prg_fgr_step(prg_fgr* h, int decrease_mu, double division_factor, double maximum_correspondence_distance);
/* `iterations` (0 .. 100000) times "sums, step" without a host round trip per iteration. */
int prg_fgr_iterate(prg_fgr* h, int iterations, int decrease_mu, double division_factor, double maximum_correspondence_distance);
/* Pose (12; with caller_units: R and scale_global t + mean_q - R mean_p), mu, the steps done, the status (0 ok, 1 fewer than
 * three used pairs, 2 degenerate) and the objective of the last sums.  Any output may be NULL.  Synchronises. */
int prg_fgr_get_state(prg_fgr* h, int caller_units, double* pose_host, double* mu_host, int64_t* n_iter_host, int* status_host,
                      double* objective_host);
/* The line-process value l of every used pair (k doubles) at the state's pose and mu.  Synchronises. */
int prg_fgr_get_weights(prg_fgr* h, double* weights_host);

#ifdef __cplusplus
}
#endif
#endif /* PROBREG_HIP_H */
