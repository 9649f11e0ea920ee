#!/usr/bin/env python
"""Time the k-NN search and the outlier filters (csrc/grid_search.hip, csrc/icp_outlier.hip) on one MI355X and write
profiles/knn_timing.txt (or --out).

Cloud: synthetic.surface(n, 0), searched against itself (queries = cloud, identity pose).  Per size:

    build      IcpPlan.set_target (validation on the host, upload, the grid levels; the call synchronises)
    knn        IcpPlan.knn(k, inf) for k in --ks between two device synchronisations, the read-back of the lists included,
               and the kernel k_icp_knn alone from the kernel trace (one wave per query)
    search     IcpPlan.search(inf): k_icp_search, k = 1, one lane per query, on the same inputs
    count      IcpPlan.radius_count(r) with r = --radius-cells cell edges of the finest level
    topk       engine.topk_sweep (brute force, fp32, k = 8) on the same cloud, up to --topk-limit points
    filters    whole preprocess.remove_statistical_outlier(20, 2.0) and remove_radius_outlier(10, r) calls from host arrays

One child process per size for the calls (host clock, median and minimum over --rounds after one warm-up) and one under
`rocprofv3 --kernel-trace` for the kernel times; each under `timeout -k 10`, and nothing is started after a child that failed.

--cpu-only: time scipy.spatial.cKDTree.query(k=20) of the cloud against itself on this host, one thread, and append the lines
to --out."""
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


def cloud_of(n):
    from probreg_amd import synthetic

    return np.ascontiguousarray(synthetic.surface(n, 0))


def clock(fn, rounds, sync):
    ts = []
    for _ in range(rounds + 1):  # the first one warms up
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts[1:]


def worker(mode, n, ks, radius_cells, topk_limit, work, rounds):
    import torch

    from probreg_amd import _lib, engine, icp, preprocess

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    cloud = cloud_of(n)
    res = {"n": n, "knn": {}}
    plan = icp.IcpPlan()
    res["build"] = clock(lambda: plan.set_target(cloud), rounds if mode == "calls" else 1, sync)
    edge, dims, dense, levels = plan.grid()
    res["grid"] = {"edge": edge, "dims": [int(d) for d in dims], "dense": dense, "levels": levels}
    plan.set_source(cloud)
    r = radius_cells * edge
    res["radius"] = r
    res["search"] = clock(lambda: plan.search(np.inf), rounds, sync)
    for k in ks:
        res["knn"][str(k)] = clock(lambda: plan.knn(k), rounds, sync)
    res["count"] = clock(lambda: plan.radius_count(r), rounds, sync)
    res["count_mean"] = float(np.mean(plan.radius_count(r)))
    plan.close()
    if mode == "calls":
        few = min(rounds, 5)
        res["statistical"] = clock(lambda: preprocess.remove_statistical_outlier(cloud, 20, 2.0), few, sync)
        res["radius_filter"] = clock(lambda: preprocess.remove_radius_outlier(cloud, 10, r), few, sync)
        if n <= topk_limit:
            x = cloud.astype(np.float32)
            res["topk"] = clock(lambda: engine.topk_sweep(x, x, 1.0, k=8), few, sync)
    with open(os.path.join(work, "%s_%d.json" % (mode, n)), "w") as f:
        json.dump(res, f)


KERNELS = ("k_icp_knn", "k_icp_search", "k_icp_radius_count", "k_knn_mean_distance", "k_outlier_runs", "k_outlier_finish",
           "k_outlier_mask", "k_icp_query_keys", "k_cell_keys", "k_cell_bounds", "k_icp_reset")


def short(name):
    for key in KERNELS:
        if key in name:
            return key
    return "other (sort)"


def traced(trace_dir):
    """name -> seconds of every launch, in launch order."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, start, end in cur.execute("select name, start, end from kernels order by start"):
            out.setdefault(short(name), []).append((end - start) * 1.0e-9)
    return out


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def cpu_lines(sizes):
    from scipy.spatial import cKDTree

    lines = ["# scipy.spatial.cKDTree on %s, one thread" % cpu_name()]
    for n in sizes:
        cloud = cloud_of(n)
        t0 = time.perf_counter()
        tree = cKDTree(cloud)
        t1 = time.perf_counter()
        tree.query(cloud, k=20, workers=1)
        t2 = time.perf_counter()
        lines.append("cKDTree, n = %d: build %.1f ms, query(k=20) of the cloud itself: %.1f ms" % (n, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    return lines


def ms(ts):
    return "%10.3f %10.3f" % (1e3 * float(np.median(ts)), 1e3 * min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 8, 20, 64])
    ap.add_argument("--radius-cells", type=float, default=2.0)
    ap.add_argument("--topk-limit", type=int, default=100000)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=200, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_timing.txt"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.n, args.ks, args.radius_cells, args.topk_limit, args.work, args.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.cpu_only:
        text = "\n".join(cpu_lines(args.sizes)) + "\n"
        print(text)
        with open(args.out, "a") as f:
            f.write(text)
        return
    work = tempfile.mkdtemp(prefix="knn_timing_")
    lines = ["# tools/knn_timing.py: surface(n, 0) searched against itself, r = inf; %d rounds after one warm-up; ms: median, "
             "minimum" % args.rounds,
             "# call: host clock around work that ends in a device synchronise (knn and count: with the read-back); kernel: one "
             "launch, from a kernel trace of its own run"]
    failed = False

    def child(mode, n, trace=None):
        cmd = ["timeout", "-k", "10", str(args.limit)]
        if trace:
            cmd += ["rocprofv3", "--kernel-trace", "-d", trace, "-o", "t", "--"]
        cmd += [sys.executable, os.path.abspath(__file__), "--worker", mode, "--n", str(n), "--work", work, "--rounds",
                str(args.rounds), "--radius-cells", repr(args.radius_cells), "--topk-limit", str(args.topk_limit), "--ks"]
        cmd += [str(k) for k in args.ks]
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
        g = res["grid"]
        lines.append("n = %d: cell edge %.5g, %d x %d x %d cells (%s), %d levels" % ((n, g["edge"]) + tuple(g["dims"])
                                                                                    + ("dense" if g["dense"] else "hashed", g["levels"])))
        lines.append("  call    %-52s %s" % ("set_target (grid build with upload)", ms(res["build"])))
        lines.append("  call    %-52s %s" % ("search(inf): k = 1, one lane per query", ms(res["search"])))
        for k in args.ks:
            lines.append("  call    %-52s %s" % ("knn(%d, inf) with read-back: one wave per query" % k, ms(res["knn"][str(k)])))
        lines.append("  call    %-52s %s   (%.1f points on average)" % ("radius_count(r = %.4g) with read-back" % res["radius"],
                                                                        ms(res["count"]), res["count_mean"]))
        lines.append("  call    %-52s %s" % ("remove_statistical_outlier(20, 2.0), host arrays", ms(res["statistical"])))
        lines.append("  call    %-52s %s" % ("remove_radius_outlier(10, r), host arrays", ms(res["radius_filter"])))
        if "topk" in res:
            lines.append("  call    %-52s %s" % ("engine.topk_sweep, fp32 brute force, k = 8", ms(res["topk"])))
        trace = os.path.join(work, "trace_%d" % n)
        if not child("kernels", n, trace):
            failed = True
            break
        times = traced(trace)
        knn = times.pop("k_icp_knn", [])
        per = args.rounds + 1
        if len(knn) == per * len(args.ks):  # per k: a warm-up launch, then the rounds
            for j, k in enumerate(args.ks):
                lines.append("  kernel  %-52s %s" % ("k_icp_knn, k = %d" % k, ms(knn[j * per + 1:(j + 1) * per])))
        elif knn:
            lines.append("  kernel  %-52s %s   (%d launches, not one set per k)" % ("k_icp_knn, every k", ms(knn), len(knn)))
        print("\n".join(lines), flush=True)
        for name, ts in sorted(times.items()):
            lines.append("  kernel  %-52s %s   (%d launches)" % (name, ms(ts), len(ts)))
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    if failed:
        print(text)
        sys.exit(1)


if __name__ == "__main__":
    main()
