#!/usr/bin/env python
"""Time ICP (csrc/icp.hip, csrc/grid_search.hip) on one MI355X and write profiles/icp_timing.txt (or --out).

Clouds: synthetic.rigid_pair(n, seed=0) at M = N = n (source and target are independent samples, the target turned by 30 and
10 degrees), the target's analytic normals for point-to-plane.  Every loop starts from the identity pose: the clouds are not
aligned, which is the start of an ICP run and the hard case of the grid search (queries far from the target walk empty cells);
the search is timed at the true pose as well.
Per size and r in --radii:

    build      IcpPlan.set_target (validation on the host, upload, the grid levels; the call synchronises)
    search     IcpPlan.search between two device synchronisations, at the identity pose and at the pose the target was made
               with (the state an ICP run ends in: every query next to its match)
    iteration  (iterate with 5 iterations - iterate with 0 iterations) / 5, stop test disabled: step, search, evaluation
    call       registration_icp from host arrays with its defaults (point-to-point, at most 30 iterations)
    sweep      the brute-force fp32 nearest-neighbour sweep behind prg_nn_mean_distance (math_utils.compute_rmse) on the
               same clouds, re-measured here

Per size one child process for the calls (host clock, median and minimum over --rounds after one warm-up) and one per
(size, r) under `rocprofv3 --kernel-trace` for the kernel times; each under `timeout -k 10`, and nothing is started after a
child that failed.

--cpu-only: time scipy.spatial.cKDTree (build, query of the same queries) on this host and append the lines to --out."""
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

KINDS = ("point_to_point", "point_to_plane")


def clouds(n):
    from probreg_amd import synthetic

    src, tgt, (rot, t, _) = synthetic.rigid_pair(n, seed=0)
    nrm = synthetic.surface_with_normals(n, 1)[1] @ rot.T  # rigid_pair draws its target as surface(n, seed + 1)
    true = np.eye(4)
    true[:3, :3], true[:3, 3] = rot, t
    return src, tgt, np.ascontiguousarray(nrm), true


def clock(fn, rounds, sync):
    ts = []
    for _ in range(rounds + 1):  # the first one warms up
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts[1:]


def worker(mode, n, radii, work, rounds):
    import torch

    from probreg_amd import _lib, icp, math_utils

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    src, tgt, nrm, true = clouds(n)
    res = {"n": n, "r": {}}
    plan = icp.IcpPlan()
    res["build"] = clock(lambda: plan.set_target(tgt, nrm), rounds if mode == "calls" else 1, sync)
    edge, dims, dense, levels = plan.grid()
    res["grid"] = {"edge": edge, "dims": [int(d) for d in dims], "dense": dense, "levels": levels}
    plan.set_source(src)

    def loop(kind, iters):
        plan.set_pose(None)
        plan.iterate(kind, r, iters, -1.0, -1.0, chunk=max(iters, 1))

    for r in radii:
        plan.set_pose(None)
        out = {"search": clock(lambda: plan.search(r), rounds, sync)}
        out["matched"] = float(np.mean(plan.matches()[0] >= 0))
        plan.set_pose(true)
        out["search_true"] = clock(lambda: plan.search(r), rounds, sync)
        out["matched_true"] = float(np.mean(plan.matches()[0] >= 0))
        for kind in KINDS:
            out[kind] = {"5": clock(lambda: loop(kind, 5), rounds, sync), "0": clock(lambda: loop(kind, 0), rounds, sync)}
        if mode == "calls":
            out["call"] = clock(lambda: icp.registration_icp(src, tgt, r), min(rounds, 5), sync)
        res["r"][repr(r)] = out
    res["sweep"] = clock(lambda: math_utils.compute_rmse(src, tgt), min(rounds, 5), sync)
    plan.close()
    with open(os.path.join(work, "%s_%d_%s.json" % (mode, n, "_".join(repr(r) for r in radii))), "w") as f:
        json.dump(res, f)


def short(name):
    for key in ("k_icp_search", "k_icp_sums", "k_icp_finish", "k_icp_step", "k_icp_reset", "k_cell_keys", "k_cell_bounds",
                "k_icp_query_keys", "k_nn_min", "k_nn_fill", "k_nn_mean"):
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


def cpu_lines(sizes, radii):
    from scipy.spatial import cKDTree

    lines = []
    for n in sizes:
        src, tgt, _, _ = clouds(n)
        t0 = time.perf_counter()
        tree = cKDTree(tgt)
        t1 = time.perf_counter()
        lines.append("scipy cKDTree on the build machine's CPU, n = %d: build %.1f ms" % (n, 1e3 * (t1 - t0)))
        for r in radii:
            t0 = time.perf_counter()
            tree.query(src, k=1, distance_upper_bound=r)
            lines.append("  query of %d points, r = %g, one thread: %.1f ms" % (n, r, 1e3 * (time.perf_counter() - t0)))
    return lines


def ms(ts):
    return "%10.3f %10.3f" % (1e3 * float(np.median(ts)), 1e3 * min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--radii", type=float, nargs="+", default=[0.05, 0.5])
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=200, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_timing.txt"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.n, args.radii, args.work, args.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.cpu_only:
        text = "\n".join(cpu_lines(args.sizes, args.radii)) + "\n"
        print(text)
        with open(args.out, "a") as f:
            f.write(text)
        return
    work = tempfile.mkdtemp(prefix="icp_timing_")
    lines = ["# tools/icp_timing.py: rigid_pair(n, seed=0), M = N = n, every loop from the identity pose; %d rounds after one "
             "warm-up; ms: median, minimum" % args.rounds,
             "# call: host clock around work that ends in a device synchronise; kernel: one launch, from a kernel trace of its own run"]
    failed = False

    def child(mode, n, radii, trace=None):
        cmd = ["timeout", "-k", "10", str(args.limit)]
        if trace:
            cmd += ["rocprofv3", "--kernel-trace", "-d", trace, "-o", "t", "--"]
        cmd += [sys.executable, os.path.abspath(__file__), "--worker", mode, "--n", str(n), "--work", work, "--rounds",
                str(args.rounds), "--radii"] + [repr(r) for r in radii]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if proc.returncode != 0:  # nothing is started on the device after a step that failed
            lines.append("# STOPPED: n = %d, %s %s ended with exit status %d.  Last output:" % (n, mode, radii, proc.returncode))
            lines.extend("#   " + s for s in proc.stdout.splitlines()[-15:])
            return False
        return True

    for n in args.sizes:
        if not child("calls", n, args.radii):
            failed = True
            break
        res = json.load(open(os.path.join(work, "calls_%d_%s.json" % (n, "_".join(repr(r) for r in args.radii)))))
        g = res["grid"]
        lines.append("n = %d: cell edge %.5g, %d x %d x %d cells (%s), %d levels" % ((n, g["edge"]) + tuple(g["dims"])
                                                                                    + ("dense" if g["dense"] else "hashed", g["levels"])))
        lines.append("  call    %-44s %s" % ("set_target (grid build with upload)", ms(res["build"])))
        lines.append("  call    %-44s %s" % ("compute_rmse (fp32 sweep with upload)", ms(res["sweep"])))
        for r in args.radii:
            c = res["r"][repr(r)]
            lines.append("  r = %g: %.1f %% of the source matched at the identity pose" % (r, 100.0 * c["matched"]))
            lines.append("  call    %-44s %s" % ("search at the identity pose", ms(c["search"])))
            lines.append("  call    %-44s %s   (%.1f %% matched)" % ("search at the true pose", ms(c["search_true"]),
                                                                    100.0 * c["matched_true"]))
            for kind in KINDS:
                per = (np.median(c[kind]["5"]) - np.median(c[kind]["0"])) / 5.0
                lines.append("  call    %-44s %10.3f" % ("one iteration, " + kind, 1e3 * per))
            lines.append("  call    %-44s %s" % ("registration_icp (whole call, host arrays)", ms(c["call"])))
            trace = os.path.join(work, "trace_%d_%r" % (n, r))
            if not child("kernels", n, [r], trace):
                failed = True
                break
            for name, ts in sorted(traced(trace).items()):
                lines.append("  kernel  %-44s %s   (%d launches)" % (name, ms(ts), len(ts)))
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
