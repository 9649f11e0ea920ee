#!/usr/bin/env python
"""Time of ``registration_cpd_batch`` against a Python loop over ``registration_cpd`` with the same arguments, on one GPU.

    python tools/cpd_batch_timing.py [--repeats 5] [--sizes 256 1000 4000] [--batches 1 16 256 1024] [--out profiles/cpd_batch_timing.txt]

Workload: rigid, ``maxiter=30``, ``tol=-1``, ``w=0.1``, problem b is ``synthetic.rigid_pair(n, n, seed=b)``.  The two paths run in the
same process, alternating (loop, batch, loop, batch ...), after one untimed run of each at every shape; both calls end with their own
read-back and a device synchronise follows, so a host clock brackets each.  Printed: median, minimum and maximum over ``--repeats``
runs and the ratio of the medians.  The loop is the single-problem path, which the batch plan leaves as it was.

Then, on the plan itself (``engine.CpdBatchPlan``: clouds already on the device, 30 iterations enqueued, one synchronise), the time per
EM iteration of the largest batch at M = N = 1000 and what that is of the chip's fp32 vector rate, counting the sweep's 21 fp32
operations per pair (3 sub, 1 mul + 2 fma for d^2, 1 min, 1 fma + 1 exp2 for K, 1 add + 4 fma for the five sums; an fma counts 2)
against 157.3 TFLOP/s.  Last, the default ``tol=1e-3`` run at B = 256, M = N = 1000 with the iterations its problems stopped at.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from probreg_amd import _lib, cpd, engine, synthetic  # noqa: E402

MAXITER = 30
W = 0.1
FLOP_PER_PAIR = 21.0
PEAK_FP32 = 157.3e12


def sync():
    import torch

    torch.cuda.synchronize()


def clouds(b, n):
    pairs = [synthetic.rigid_pair(n, n, seed=s)[:2] for s in range(b)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def run_loop(srcs, tgts, tol):
    out = [cpd.registration_cpd(s, t, "rigid", w=W, maxiter=MAXITER, tol=tol) for s, t in zip(srcs, tgts)]
    sync()
    return out


def run_batch(srcs, tgts, tol):
    out = cpd.registration_cpd_batch(srcs, tgts, "rigid", w=W, maxiter=MAXITER, tol=tol, return_n_iter=True)
    sync()
    return out


def timed(fn, *a):
    t0 = time.perf_counter()
    fn(*a)
    return time.perf_counter() - t0


def fmt(v):
    v = np.asarray(v) * 1e3
    return "%10.3f ms (min %10.3f, max %10.3f)" % (np.median(v), v.min(), v.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1000, 4000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("registration_cpd_batch vs a loop over registration_cpd: rigid, maxiter=%d, tol=-1, w=%.1f, %d repeats (median, min, max)"
        % (MAXITER, W, args.repeats))
    say("%6s %6s  %-44s %-44s %8s" % ("M=N", "B", "loop over registration_cpd", "registration_cpd_batch", "loop/batch"))
    for n in args.sizes:
        src_all, tgt_all = clouds(max(args.batches), n)
        for b in args.batches:
            srcs, tgts = src_all[:b], tgt_all[:b]
            run_loop(srcs, tgts, -1)
            run_batch(srcs, tgts, -1)  # warm-up of both at this shape
            tl, tb = [], []
            for _ in range(args.repeats):
                tl.append(timed(run_loop, srcs, tgts, -1))
                tb.append(timed(run_batch, srcs, tgts, -1))
            say("%6d %6d  %-44s %-44s %8.1fx" % (n, b, fmt(tl), fmt(tb), np.median(tl) / np.median(tb)))

    # the sweep alone: clouds on the device, 30 iterations enqueued back to back, one synchronise
    n, b = 1000, max(args.batches)
    srcs, tgts = clouds(b, n)
    plan = engine.CpdBatchPlan([s - s.mean(axis=0) for s in srcs], [t - t.mean(axis=0) for t in tgts])
    wv, tolv = np.full(b, W), np.full(b, -1.0)
    ts = []
    for r in range(args.repeats + 1):
        plan.init(None)
        plan.active()  # (synchronises)
        t0 = time.perf_counter()
        plan.iterate(_lib.PRG_TF_RIGID, True, wv, tolv, MAXITER)
        plan.active()
        if r > 0:
            ts.append((time.perf_counter() - t0) / MAXITER)
    plan.close()
    per_it = float(np.median(ts))
    pairs = float(b) * n * n
    say("")
    say("plan only, B=%d, M=N=%d: %.1f us per EM iteration of the whole batch (min %.1f, max %.1f; sweep + M-step launches), "
        "%.3g pairs -> %.2f TFLOP/s at %d fp32 operations per pair = %.1f %% of the %.1f TFLOP/s fp32 vector peak"
        % (b, n, per_it * 1e6, min(ts) * 1e6, max(ts) * 1e6, pairs, pairs * FLOP_PER_PAIR / per_it / 1e12, int(FLOP_PER_PAIR),
           100.0 * pairs * FLOP_PER_PAIR / per_it / PEAK_FP32, PEAK_FP32 / 1e12))

    # the default tolerance
    n, b = 1000, 256
    srcs, tgts = clouds(b, n)
    run_loop(srcs[:2], tgts[:2], 1e-3)
    _, n_iter = run_batch(srcs, tgts, 1e-3)
    tl, tb = [], []
    for _ in range(args.repeats):
        tl.append(timed(run_loop, srcs, tgts, 1e-3))
        tb.append(timed(run_batch, srcs, tgts, 1e-3))
    say("")
    say("default tol=1e-3, maxiter=%d, B=%d, M=N=%d: loop %s   batch %s   %.1fx" % (MAXITER, b, n, fmt(tl), fmt(tb),
                                                                                   np.median(tl) / np.median(tb)))
    say("  n_iter of the batch: min %d, median %d, max %d (%d of %d problems stopped before maxiter)"
        % (n_iter.min(), int(np.median(n_iter)), n_iter.max(), int(np.sum(n_iter < MAXITER)), b))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
