#!/usr/bin/env python
"""Time generalized ICP (csrc/icp.hip, its search in csrc/grid_search.hip) on one MI355X and write profiles/gicp_timing.txt (or --out).

Clouds: synthetic.pt2pl_pair(n, seed=0) at M = N = n with the analytic normals of both clouds (the source's rounded through
float32 as the target's are), epsilon = 1e-3, r = --radius.  Every loop starts from the identity pose, 12 and 6 degrees from the
pose the target was made with.  Per size, for the generalized estimator and, on the same plan in the same run, point-to-plane:

    iteration  (iterate with 5 iterations - iterate with 0 iterations) / 5, stop test disabled: step, search, evaluation
    kernels    5-iteration loops under `rocprofv3 --kernel-trace`, in a run of their own per estimator: per loop the time
               of all its launches of search (k_icp_search, 6: the evaluation of the start pose and one per iteration), sums
               (k_icp_sums and k_icp_finish, 6 each) and step (k_icp_step, 5), divided by 5; medians over the loops.  The
               poses of the loop are the estimator's own, so its search times are too.
    setup      set_source_covariances / set_target_covariances from normals (upload, kernel, synchronise)

One child process per measurement, each under `timeout -k 10`; nothing is started after a child that failed."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("generalized", "point_to_plane")
ITERS = 5
# bytes one matched pair makes the generalized sums read: source point, index, d2, source covariance, target point (padded),
# target covariance
PAIR_BYTES = 24 + 4 + 8 + 48 + 32 + 48


def clouds(n):
    from probreg_amd import synthetic

    src, tgt, tn, _ = synthetic.pt2pl_pair(n, seed=0)
    sn = synthetic.surface_with_normals(n, 0)[1].astype(np.float32).astype(np.float64)
    return src, tgt, sn, tn


def clock(fn, rounds, sync):
    ts = []
    for _ in range(rounds + 1):  # the first one warms up
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts[1:]


def worker(mode, n, r, work, rounds):
    import torch

    from probreg_amd import _lib, icp

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    src, tgt, sn, tn = clouds(n)
    plan = icp.IcpPlan()
    plan.set_target(tgt, tn)
    plan.set_source(src)
    res = {"n": n}
    if mode == "calls":
        res["cov_source"] = clock(lambda: plan.set_source_covariances(normals=sn), rounds, sync)
        res["cov_target"] = clock(lambda: plan.set_target_covariances(normals=tn), rounds, sync)
    else:
        plan.set_source_covariances(normals=sn)
        plan.set_target_covariances(normals=tn)

    def loop(kind, iters):
        plan.set_pose(None)
        plan.iterate(kind, r, iters, -1.0, -1.0, chunk=max(iters, 1))

    for kind in KINDS if mode == "calls" else (mode,):
        res[kind] = {"5": clock(lambda: loop(kind, ITERS), rounds, sync)}
        if mode == "calls":
            res[kind]["0"] = clock(lambda: loop(kind, 0), rounds, sync)
    res["matched"] = float(np.mean(plan.matches()[0] >= 0))
    plan.close()
    with open(os.path.join(work, "%s_%d.json" % (mode, n)), "w") as f:
        json.dump(res, f)


def short(name):
    for mode in "0123":
        if "k_icp_sums<%s>" % mode in name or "k_icp_sumsILi%sE" % mode in name:
            return "k_icp_sums<%s>" % mode
    for key in ("k_icp_search", "k_icp_sums", "k_icp_finish", "k_icp_step", "k_icp_reset", "k_icp_query_keys",
                "k_icp_cov_from_normals", "k_cell_keys", "k_cell_bounds"):
        if key in name:
            return key
    return "sort (rocPRIM)"


def traced(trace_dir):
    """name -> seconds of every launch, in launch order."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, start, end in cur.execute("select name, start, end from kernels order by start"):
            out.setdefault(short(name), []).append((end - start) * 1.0e-9)
    return out


def med(ts):
    return 1e3 * float(np.median(ts))


def per_iteration(ts, loops, launches):
    """ms per iteration: `ts` holds `launches` launches for each of `loops` loops, the first loop warms up."""
    if len(ts) != loops * launches:
        raise RuntimeError("expected %d x %d launches, the trace has %d" % (loops, launches, len(ts)))
    return 1e3 * float(np.median(np.sum(np.reshape(ts, (loops, launches)), axis=1)[1:])) / ITERS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--radius", type=float, default=0.05)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=150, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_timing.txt"))
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.n, args.radius, args.work, args.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    work = tempfile.mkdtemp(prefix="gicp_timing_")
    lines = ["# tools/gicp_timing.py: pt2pl_pair(n, seed=0), M = N = n, r = %g, epsilon = 1e-3, every loop from the identity pose; "
             "%d rounds after one warm-up; ms, medians" % (args.radius, args.rounds),
             "# call: host clock around work that ends in a device synchronise; kernel: per iteration of a %d-iteration loop (stop test "
             "disabled; the loop's launches / %d, the evaluation of the start pose included), from a kernel trace of its own run"
             % (ITERS, ITERS)]
    failed = False

    def child(mode, n, trace=None):
        cmd = ["timeout", "-k", "10", str(args.limit)]
        if trace:
            cmd += ["rocprofv3", "--kernel-trace", "-d", trace, "-o", "t", "--"]
        cmd += [sys.executable, os.path.abspath(__file__), "--worker", mode, "--n", str(n), "--work", work, "--rounds",
                str(args.rounds), "--radius", repr(args.radius)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if proc.returncode != 0:  # nothing is started on the device after a step that failed
            lines.append("# STOPPED: n = %d, %s ended with exit status %d.  Last output:" % (n, mode, proc.returncode))
            lines.extend("#   " + s for s in proc.stdout.splitlines()[-15:])
            return False
        return True

    for n in args.sizes:
        if not child("calls", n):
            failed = True
            break
        res = json.load(open(os.path.join(work, "calls_%d.json" % n)))
        lines.append("n = %d: %.1f %% of the source matched at the identity pose" % (n, 100.0 * res["matched"]))
        lines.append("  call    %-52s %8.3f / %.3f" % ("covariances from normals, source / target", med(res["cov_source"]),
                                                        med(res["cov_target"])))
        for kind in KINDS:
            per = (np.median(res[kind]["5"]) - np.median(res[kind]["0"])) / ITERS
            lines.append("  call    %-52s %8.3f" % ("one iteration, " + kind, 1e3 * per))
        for kind in KINDS:
            trace = os.path.join(work, "trace_%d_%s" % (n, kind))
            if not child(kind, n, trace):
                failed = True
                break
            k = traced(trace)
            sums = "k_icp_sums<3>" if kind == "generalized" else "k_icp_sums<2>"
            if sums not in k:  # the trace names the kernel without its template argument
                sums = "k_icp_sums"
            loops = args.rounds + 1
            parts = {"search": per_iteration(k["k_icp_search"], loops, ITERS + 1), "sums": per_iteration(k[sums], loops, ITERS + 1),
                     "finish": per_iteration(k["k_icp_finish"], loops, ITERS + 1),
                     "step": per_iteration(k["k_icp_step"], loops, ITERS)}
            end = json.load(open(os.path.join(work, "%s_%d.json" % (kind, n))))["matched"]
            one = 1e3 * k[sums][-1]  # the evaluation that ends the last loop
            total = sum(parts.values())
            lines.append("  kernel  %-52s search %.4f, sums %.4f (%s) + %.4f (k_icp_finish), step %.4f: %.4f; the sums kernel is "
                         "%.1f %% of it" % (kind + ", the kernels of one iteration", parts["search"], parts["sums"], sums,
                                            parts["finish"], parts["step"], total, 100.0 * parts["sums"] / total))
            if kind == "generalized":
                rate = end * n * PAIR_BYTES / (one * 1.0e-3)
                lines.append("  kernel  %-52s %.4f ms with %.1f %% matched: %.1f MB read for the pairs, %.3f TB/s; %d lanes (one per "
                             "run of 64 source points)" % ("the last launch of k_icp_sums<3>", one, 100.0 * end,
                                                           end * n * PAIR_BYTES / 1e6, rate / 1e12, -(-n // 64)))
        if failed:
            break
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
