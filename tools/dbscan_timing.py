#!/usr/bin/env python
"""Time DBSCAN (csrc/icp_cluster.hip) on one MI355X and write profiles/dbscan_timing.txt (or --out).

Clouds: synthetic.surface(n, 0), and the scene of the tests (three surfaces of 900 : 600 : 300 points and 80 uniform outliers
per 1880, permuted) scaled to n points.  eps = --eps-cells cell edges of the finest level of the cloud's grid, min_points = 10.
Per cloud:

    call     IcpPlan.radius_count(eps) and IcpPlan._dbscan(eps, min_points) on a plan that holds the cloud, with their read-backs,
             and the whole preprocess.cluster_dbscan(cloud, eps, min_points) from a host array, on a host clock between device
             synchronisations; the first call of each is a warm-up and is reported apart
    kernel   every kernel of _dbscan from a kernel trace of a run of its own: k_icp_radius_count (the count), k_dbscan_core,
             k_dbscan_link (the same walk with the union-find), k_dbscan_root_count / tile_scan / number / label (flatten and number)

One child process per cloud and kind, each under `timeout -k 10`; nothing is started after a child that failed.  Medians and
minima over --rounds.

--cpu-only: sklearn.cluster.DBSCAN (its default neighbour search, one job) on this host at the sizes up to --cpu-limit, with the
eps the GPU run used (read from --out, where it appends its lines)."""
import argparse
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIN_POINTS = 10


def cloud_of(kind, n):
    from probreg_amd import synthetic

    if kind == "surface":
        return np.ascontiguousarray(synthetic.surface(n, 0))
    na, nb, nc = (n * 900) // 1880, (n * 600) // 1880, (n * 300) // 1880
    rng = np.random.default_rng(0)
    parts = [synthetic.surface(na, 11), 0.8 * synthetic.surface(nb, 12) + np.array([3.0, 0.2, 0.1]),
             0.6 * synthetic.surface(nc, 13) + np.array([0.3, 2.4, 0.9]),
             rng.uniform((-1.6, -1.0, -0.8), (4.2, 3.2, 1.6), (n - na - nb - nc, 3))]
    cloud = np.concatenate(parts, axis=0)
    return np.ascontiguousarray(cloud[rng.permutation(n)])


def clock(fn, rounds, sync):
    ts = []
    for _ in range(rounds + 1):  # the first one warms up and is kept apart
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts


def worker(mode, kind, n, eps_cells, work, rounds):
    import torch

    from probreg_amd import _lib, icp, preprocess

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    cloud = cloud_of(kind, n)
    plan = icp.IcpPlan()
    plan.set_target(cloud)
    plan.set_source(cloud)
    edge, dims, dense, levels = plan.grid()
    eps = eps_cells * edge
    res = {"n": n, "eps": eps, "grid": {"edge": edge, "dims": [int(d) for d in dims], "dense": dense, "levels": levels}}
    res["count"] = clock(lambda: plan.radius_count(eps), rounds, sync)
    res["dbscan"] = clock(lambda: plan._dbscan(eps, MIN_POINTS), rounds, sync)
    labels, core, counts, n_clusters, sizes = plan._dbscan(eps, MIN_POINTS)
    plan.close()
    res["result"] = {"clusters": n_clusters, "largest": [int(s) for s in np.sort(sizes)[::-1][:4]], "core": int(core.sum()),
                     "noise": int(np.sum(labels < 0)), "count_mean": float(np.mean(counts))}
    if mode == "calls":
        res["public"] = clock(lambda: preprocess.cluster_dbscan(cloud, eps, MIN_POINTS), min(rounds, 5), sync)
    with open(os.path.join(work, "%s_%s_%d.json" % (mode, kind, n)), "w") as f:
        json.dump(res, f)


KERNELS = ("k_icp_radius_count", "k_dbscan_core", "k_dbscan_link", "k_dbscan_root_count", "k_dbscan_tile_scan", "k_dbscan_number",
           "k_dbscan_label")


def traced(trace_dir):
    """name -> seconds of every launch, in launch order."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, start, end in cur.execute("select name, start, end from kernels order by start"):
            for key in KERNELS:
                if key in name:
                    out.setdefault(key, []).append((end - start) * 1.0e-9)
    return out


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def cpu_lines(out, limit):
    from sklearn.cluster import DBSCAN

    cases = re.findall(r"^(surface|scene), n = (\d+): eps = ([0-9.eE+-]+),", open(out).read(), flags=re.M)
    lines = ["# sklearn.cluster.DBSCAN(eps, min_samples = %d), default neighbour search, n_jobs = 1, on %s" % (MIN_POINTS, cpu_name())]
    for kind, n, eps in cases:
        if int(n) > limit:
            continue
        cloud = cloud_of(kind, int(n))
        t0 = time.perf_counter()
        sk = DBSCAN(eps=float(eps), min_samples=MIN_POINTS, n_jobs=1).fit(cloud)
        t1 = time.perf_counter()
        lines.append("sklearn DBSCAN, %s, n = %s, eps = %s: %.1f ms, %d clusters, %d core, %d noise"
                     % (kind, n, eps, 1e3 * (t1 - t0), int(sk.labels_.max()) + 1, sk.core_sample_indices_.shape[0],
                        int(np.sum(sk.labels_ < 0))))
    return lines


def ms(ts):
    return "%10.3f %10.3f" % (1e3 * float(np.median(ts)), 1e3 * min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--kinds", nargs="+", default=["surface", "scene"])
    ap.add_argument("--eps-cells", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--limit", type=int, default=200, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_timing.txt"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--cpu-limit", type=int, default=100000)
    ap.add_argument("--worker")
    ap.add_argument("--kind")
    ap.add_argument("--n", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.kind, args.n, args.eps_cells, args.work, args.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.cpu_only:
        text = "\n".join(cpu_lines(args.out, args.cpu_limit)) + "\n"
        print(text)
        with open(args.out, "a") as f:
            f.write(text)
        return
    work = tempfile.mkdtemp(prefix="dbscan_timing_")
    lines = ["# tools/dbscan_timing.py: eps = %g cell edges of the finest level, min_points = %d; %d rounds after one warm-up "
             "(given apart); ms: median, minimum" % (args.eps_cells, MIN_POINTS, args.rounds),
             "# call: host clock around work that ends in a device synchronise, read-backs included; kernel: one launch, from a "
             "kernel trace of its own run"]
    failed = False

    def child(mode, kind, n, trace=None):
        cmd = ["timeout", "-k", "10", str(args.limit)]
        if trace:
            cmd += ["rocprofv3", "--kernel-trace", "-d", trace, "-o", "t", "--"]
        cmd += [sys.executable, os.path.abspath(__file__), "--worker", mode, "--kind", kind, "--n", str(n), "--work", work,
                "--rounds", str(args.rounds), "--eps-cells", repr(args.eps_cells)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if proc.returncode != 0:  # nothing is started on the device after a step that failed
            lines.append("# STOPPED: %s, n = %d, %s ended with exit status %d.  Last output:" % (kind, n, mode, proc.returncode))
            lines.extend("#   " + s for s in proc.stdout.splitlines()[-15:])
            return False
        return True

    for kind in args.kinds:
        for n in args.sizes:
            if failed or not child("calls", kind, n):
                failed = True
                break
            res = json.load(open(os.path.join(work, "calls_%s_%d.json" % (kind, n))))
            g, r = res["grid"], res["result"]
            lines.append("%s, n = %d: eps = %.6g, cell edge %.5g, %d x %d x %d cells (%s), %d levels"
                         % ((kind, n, res["eps"], g["edge"]) + tuple(g["dims"]) + ("dense" if g["dense"] else "hashed", g["levels"])))
            lines.append("  result  %d clusters (largest %s), %d core, %d noise, %.1f neighbours on average"
                         % (r["clusters"], r["largest"], r["core"], r["noise"], r["count_mean"]))
            for key, what in (("count", "radius_count(eps) with read-back"), ("dbscan", "_dbscan(eps, 10) with read-back, count included"),
                              ("public", "cluster_dbscan(cloud, eps, 10), host array")):
                lines.append("  call    %-52s %s   (warm-up %.3f)" % (what, ms(res[key][1:]), 1e3 * res[key][0]))
            trace = os.path.join(work, "trace_%s_%d" % (kind, n))
            if not child("kernels", kind, n, trace):
                failed = True
                break
            times = traced(trace)
            # the worker launches the count rounds + 1 times alone, then rounds + 2 times inside _dbscan
            alone = times.get("k_icp_radius_count", [])[1:args.rounds + 1]
            if alone:
                lines.append("  kernel  %-52s %s" % ("k_icp_radius_count (alone)", ms(alone)))
            for key in KERNELS[1:]:
                ts = times.get(key, [])
                if len(ts) > 1:
                    lines.append("  kernel  %-52s %s   (%d launches, first %.3f)" % (key, ms(ts[1:]), len(ts), 1e3 * ts[0]))
            link = times.get("k_dbscan_link", [])
            if alone and len(link) > 1:
                lines.append("  ratio   %-52s %10.2f" % ("k_dbscan_link / k_icp_radius_count (medians)",
                                                        float(np.median(link[1:])) / float(np.median(alone))))
            print("\n".join(lines), flush=True)
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    if failed:
        print(text)
        sys.exit(1)


if __name__ == "__main__":
    main()
