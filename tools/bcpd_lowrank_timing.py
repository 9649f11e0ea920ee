#!/usr/bin/env python
"""BCPD with the dense kernel matrix against its pivoted-Cholesky factor: factor time, rank, M-step time
and one EM iteration on `surface` clouds of extent 2.2 with lmd = 2.  Output kept in profiles/bcpd_lowrank_timing.txt.

    python tools/bcpd_lowrank_timing.py                       # the table: dense and low-rank at 5k, 10k, 30k; low-rank alone at 1e5, 1e6
    python tools/bcpd_lowrank_timing.py --sizes 5000 10000    # other sizes (dense runs up to --dense-max, default 30000)

The split of the low-rank M-step into its kernels comes from a kernel trace of a worker that does nothing but M-steps:

    rocprofv3 --kernel-trace --stats -d DIR -o b -- python tools/bcpd_lowrank_timing.py --worker 100000
    python tools/bcpd_lowrank_timing.py --summarise DIR/<host>/<pid>_results.db 100000 <rank the worker printed>
"""
import argparse
import os
import sqlite3
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LMD = 2.0
CFAC = 1.0e3                 # s^2 / sigma2^2 of a middle iteration
WORKER_SOLVES = 6
FP64_MATRIX_PEAK = 78.6e12   # MI355X data sheet, flop/s on v_mfma_f64_16x16x4_f64

GROUPS = (("gram", ("k_lr_gram", "k_lr_gram_reduce", "k_bcpd_rhs")),
          ("cholesky", ("k_potrf_inv", "k_trsm_rows", "k_gemm_nt_f64", "k_tri_solve3", "k_fwd_update", "k_bwd_update",
                        "k_diag_solve")),
          ("v_hat", ("k_lr_apply", "k_unsort_rows")),
          ("diag_sigma", ("k_tri_inverse", "k_lr_sigma_diag")))


def _inputs(m):
    from probreg_amd import synthetic

    src = synthetic.surface(m, 1)
    rng = np.random.default_rng(m)
    nu = rng.uniform(0.0, 2.0, m)
    nu[rng.choice(m, m // 12, replace=False)] = 0.0
    return src - src.mean(axis=0), nu, rng.normal(0.0, 0.05, (m, 3))


def _sync():
    import torch

    torch.cuda.synchronize()


def _plan(src, mode):
    from probreg_amd import engine

    plan = engine.CpdPlan()
    plan.set_source(src)
    plan.bcpd_set_solver(mode, 0, 0.0)
    _sync()
    t0 = time.perf_counter()
    plan.bcpd_build_g(1.0)
    plan.synchronize()
    return plan, time.perf_counter() - t0


def _solve_ms(plan, nu, resid, repeats=3):
    best = None
    for _ in range(repeats + 1):   # the first call allocates the workspace
        t0 = time.perf_counter()
        plan.bcpd_solve(LMD, CFAC, resid, nu)   # synchronous: returns with v_hat and diag Sigma on the host
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def _em_iteration_ms(m, solver):
    """Third of three iterations of a whole registration (E-step, M-step, host algebra), N = M."""
    from probreg_amd import bcpd, synthetic

    src, tgt = synthetic.nonrigid_pair(m, seed=1)[:2]
    stamps = []
    reg = bcpd.CombinedBCPD(src, lmd=LMD, solver=solver)
    reg.set_callbacks([lambda tr: (_sync(), stamps.append(time.perf_counter()))])
    try:
        reg.registration(tgt, w=0.1, maxiter=3, tol=-1.0)
    finally:
        reg._close_plan()
    return (stamps[2] - stamps[1]) * 1e3


def table(sizes, dense_max):
    print("# BCPD M-step: dense kernel matrix (prg_cpd_bcpd_solve as before) against the factor G = F F^T; surface clouds,")
    print("# extent 2.2, c = 1, lmd = %g, cfac = %g, kernel_tol 1e-11; times in ms, best of 3 (M-step: one synchronous" % (LMD, CFAC))
    print("# prg_cpd_bcpd_solve with its uploads and read-backs); EM = third iteration of a registration with N = M")
    print("%9s | %10s %10s %10s | %10s %5s %10s %10s" % ("M", "dense G", "dense M", "dense EM", "factor", "rank", "lowrank M",
                                                         "lowrank EM"))
    for m in sizes:
        src, nu, resid = _inputs(m)
        cols = ["-", "-", "-"]
        if m <= dense_max:
            plan, t_build = _plan(src, 0)
            try:
                cols = ["%.1f" % (t_build * 1e3), "%.2f" % _solve_ms(plan, nu, resid), "%.1f" % _em_iteration_ms(m, "dense")]
            finally:
                plan.close()
        plan, t_factor = _plan(src, 1)
        try:
            rank = plan.nonrigid_rank()
            t_low = _solve_ms(plan, nu, resid)
        finally:
            plan.close()
        print("%9d | %10s %10s %10s | %10.1f %5d %10.2f %10.1f" % (m, cols[0], cols[1], cols[2], t_factor * 1e3, rank, t_low,
                                                                  _em_iteration_ms(m, "lowrank")), flush=True)


def worker(m):
    src, nu, resid = _inputs(m)
    plan, _ = _plan(src, 1)
    try:
        for _ in range(WORKER_SOLVES):
            plan.bcpd_solve(LMD, CFAC, resid, nu)
        print("worker: M=%d rank=%d, %d M-steps" % (m, plan.nonrigid_rank(), WORKER_SOLVES))
    finally:
        plan.close()


def summarise(db, m, rank):
    rows = sqlite3.connect(db).cursor().execute("select name, count(*), sum(end-start) from kernels group by name").fetchall()
    per = {}
    for name, calls, total in rows:
        short = name.replace("(anonymous namespace)::", "").replace("prg::", "").replace("void ", "").split("(")[0].split("<")[0]
        per[short] = (calls, total / 1e3 / WORKER_SOLVES)   # us per M-step
    print("# low-rank M-step at M = %d (rank %d): device time per M-step by kernel group, us (kernel trace, %d M-steps)"
          % (m, rank, WORKER_SOLVES))
    seen = set()
    for group, names in GROUPS:
        parts = [(n, per[n]) for n in names if n in per]
        seen.update(n for n, _ in parts)
        print("%-11s %10.1f   %s" % (group, sum(p[1] for _, p in parts),
                                     ", ".join("%s %.1f (x%d)" % (n, p[1], p[0] // WORKER_SOLVES) for n, p in parts)))
    if "k_lr_sigma_diag" in per and rank:
        t = per["k_lr_sigma_diag"][1] * 1e-6
        flop = float(m) * rank * rank   # 2 M r (r + 1) / 2: the lower triangle of L^-1 against every point
        print("k_lr_sigma_diag: %.3g flop in %.3f ms = %.2f Tflop/s, %.1f %% of the fp64 matrix-core peak (%.1f Tflop/s)"
              % (flop, t * 1e3, flop / t / 1e12, 100.0 * flop / t / FP64_MATRIX_PEAK, FP64_MATRIX_PEAK / 1e12))
    other = [(n, p) for n, p in per.items() if n not in seen and not n.startswith("k_pchol")]
    print("other       %10.1f   %s" % (sum(p[1] for _, p in other), ", ".join("%s %.1f" % (n, p[1]) for n, p in other)))
    fac = [(n, p) for n, p in per.items() if n.startswith("k_pchol")]
    print("(factor, once per source: %.1f ms in %d launches)" % (sum(p[1] for _, p in fac) * WORKER_SOLVES / 1e3,
                                                               sum(p[0] for _, p in fac)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[5000, 10000, 30000, 100000, 1000000])
    ap.add_argument("--dense-max", type=int, default=30000)
    ap.add_argument("--worker", type=int)
    ap.add_argument("--summarise", nargs=3, metavar=("DB", "M", "RANK"))
    a = ap.parse_args()
    if a.worker:
        worker(a.worker)
    elif a.summarise:
        summarise(a.summarise[0], int(a.summarise[1]), int(a.summarise[2]))
    else:
        table(a.sizes, a.dense_max)


if __name__ == "__main__":
    main()
