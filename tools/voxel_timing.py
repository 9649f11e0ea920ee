#!/usr/bin/env python
"""Time voxel down-sampling (csrc/voxel.hip) on one MI355X and write profiles/voxel_timing.txt (or --out).

Clouds: synthetic.surface(n, 0) at n = 10^5 and 10^6, coordinates only (d = 3, no channels).  Cases per cloud:

    ten       the voxel size that leaves about 10 points per voxel (bisection on the host)
    one       four times the largest extent: one voxel holds every point
    alone     the finest grid the 2^21 cells per axis allow (largest extent / (2^21 - 2)): nearly every point is alone; the
              number of voxels is reported

Per size two child processes, each under `timeout -k 10`; the second is started only when the first ended well:
  calls     `VoxelPlan.run` (between two device synchronisations; the cloud is already on the device) and the whole
            `voxel_down_sample` (upload, run, read-back) on a host clock: median and minimum over --rounds after one warm-up
  kernels   the same runs under `rocprofv3 --kernel-trace`: the launches are cut into runs at k_minmax_part, the kernels of a run
            are added up per stage, and the median over the runs of a case is reported

Bytes: the least traffic of a stage as DESIGN.md 3.14 counts it (d = 3; the sort at 8 bits per pass).  The share of HBM bandwidth
is those bytes over the stage's median time over 8 TB/s (the MI355X's peak; about 6.3 TB/s are achievable).

--cpu-only: time the NumPy restatement (tests/oracle_voxel.py) on this host for the case `ten` and append the lines to --out."""
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

HBM_PEAK = 8.0e12
CASES = ("ten", "one", "alone")
STAGES = ("box", "keys", "sort", "rows", "sums")
MAX_CELLS = 1 << 21


def cloud(n):
    from probreg_amd import synthetic

    return np.ascontiguousarray(synthetic.surface(n, 0))


def n_voxels(points, v):
    c = np.floor((points - (points.min(axis=0) - 0.5 * v)) / v).astype(np.int64)
    return np.unique((c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]).shape[0]


def voxel_size(points, case):
    extent = float(np.max(points.max(axis=0) - points.min(axis=0)))
    if case == "one":
        return 4.0 * extent
    if case == "alone":
        return extent / (MAX_CELLS - 2)
    lo, hi = extent / 4096.0, extent  # bisection on log v for n / V = 10
    for _ in range(30):
        mid = (lo * hi) ** 0.5
        if points.shape[0] / float(n_voxels(points, mid)) < 10.0:
            lo = mid
        else:
            hi = mid
    return hi


def key_bits(points, v):
    c = np.floor((points.max(axis=0) - (points.min(axis=0) - 0.5 * v)) / v).astype(np.int64)
    return max(1, sum(int(x).bit_length() for x in c))


def stage_bytes(n, n_vox, bits, d=3):
    """The least bytes every stage moves."""
    passes = (bits + 7) // 8
    return {"box": 8.0 * d * n,
            "keys": (8.0 * d + 12.0) * n,
            "sort": (8.0 + 24.0 * passes) * n,
            "rows": (8.0 + 20.0) * n + 4.0 * n_vox,
            "sums": (8.0 * d + 4.0) * n + (8.0 * d + 12.0) * n_vox + 4.0 * 8.0 * d * n / 64.0}


def worker(mode, n, work, rounds):
    import torch

    from probreg_amd import _lib, preprocess

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    points = cloud(n)
    res = {"n": n, "cases": {}}
    plan = preprocess.VoxelPlan()
    plan.set_data(points)
    for case in CASES:
        v = voxel_size(points, case)
        run_ts, call_ts = [], []
        for r in range(rounds + 1):  # the first one warms up
            sync()
            t0 = time.perf_counter()
            plan.run(v)
            sync()
            run_ts.append(time.perf_counter() - t0)
        n_vox = plan.count()
        if mode == "calls":
            for r in range(rounds + 1):
                t0 = time.perf_counter()
                out = preprocess.voxel_down_sample(points, v)
                call_ts.append(time.perf_counter() - t0)
            assert out.points.shape[0] == n_vox
        res["cases"][case] = {"v": v, "V": n_vox, "bits": key_bits(points, v), "run": run_ts[1:], "call": call_ts[1:]}
    plan.close()
    with open(os.path.join(work, "%s_%d.json" % (mode, n)), "w") as f:
        json.dump(res, f)


def stage_of(name):
    if "k_minmax" in name:
        return "box"
    if "k_keys" in name:
        return "keys"
    if "k_head_count" in name or "k_tile_scan" in name or "k_rows" in name:
        return "rows"
    if "k_block_pieces" in name or "k_voxel_means" in name:
        return "sums"
    return "sort"  # everything else the runs launch is rocPRIM's


def traced_runs(trace_dir):
    """Per run (cut at k_minmax_part) the seconds of every stage, in launch order."""
    runs = []
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, start, end in cur.execute("select name, start, end from kernels order by start"):
            if "k_minmax_part" in name:
                runs.append(dict.fromkeys(STAGES, 0.0))
            if runs:
                runs[-1][stage_of(name)] += (end - start) * 1.0e-9
    return runs


def cpu_lines(sizes):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_voxel as ov

    lines = []
    for n in sizes:
        points = cloud(n)
        v = voxel_size(points, "ten")
        t0 = time.perf_counter()
        ref = ov.down_sample(points, v)
        lines.append("NumPy restatement (tests/oracle_voxel.py) on the build machine's CPU, n = %d, case ten (V = %d): %.2f s"
                     % (n, ref["counts"].shape[0], time.perf_counter() - t0))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=int, default=200, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_timing.txt"))
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.n, args.work, args.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.cpu_only:
        text = "\n".join(cpu_lines(args.sizes)) + "\n"
        print(text)
        with open(args.out, "a") as f:
            f.write(text)
        return
    work = tempfile.mkdtemp(prefix="voxel_timing_")
    lines = ["# tools/voxel_timing.py: surface(n, 0), d = 3, no channels; %d rounds per case after one warm-up; ms: median, minimum"
             % args.rounds,
             "# stages: kernel time of one run from a kernel trace, median over the runs; bytes: the least traffic of the stage "
             "(DESIGN.md 3.14); share: bytes / median time / 8 TB/s"]
    failed = False
    for n in args.sizes:
        for mode in ("calls", "kernels"):
            cmd = ["timeout", "-k", "10", str(args.limit)]
            if mode == "kernels":
                cmd += ["rocprofv3", "--kernel-trace", "-d", os.path.join(work, "trace_%d" % n), "-o", "t", "--"]
            cmd += [sys.executable, os.path.abspath(__file__), "--worker", mode, "--n", str(n), "--work", work,
                    "--rounds", str(args.rounds)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
            if proc.returncode != 0:  # nothing is started on the device after a step that failed
                lines.append("# STOPPED: n = %d, %s ended with exit status %d.  Last output:" % (n, mode, proc.returncode))
                lines += ["#   " + s for s in proc.stdout.splitlines()[-15:]]
                failed = True
                break
        if failed:
            break
        calls = json.load(open(os.path.join(work, "calls_%d.json" % n)))["cases"]
        runs = traced_runs(os.path.join(work, "trace_%d" % n))
        per_case = args.rounds + 1
        for i, case in enumerate(CASES):
            c = calls[case]
            lines.append("n = %d, case %s: voxel_size = %.6g, V = %d (%.2f points per voxel), %d key bits"
                         % (n, case, c["v"], c["V"], n / float(c["V"]), c["bits"]))
            lines.append("  call   %-36s %10.3f %10.3f" % ("voxel_down_sample (whole call)", 1e3 * np.median(c["call"]), 1e3 * min(c["call"])))
            lines.append("  call   %-36s %10.3f %10.3f" % ("VoxelPlan.run", 1e3 * np.median(c["run"]), 1e3 * min(c["run"])))
            mine = runs[i * per_case + 1:(i + 1) * per_case]
            if len(runs) != len(CASES) * per_case or not mine:
                lines.append("  (the trace holds %d runs, %d were expected: no stage times)" % (len(runs), len(CASES) * per_case))
                continue
            need = stage_bytes(n, c["V"], c["bits"])
            total_t = total_b = 0.0
            for stage in STAGES:
                ts = [r[stage] for r in mine]
                med = float(np.median(ts))
                total_t += med
                total_b += need[stage]
                lines.append("  stage  %-36s %10.3f %10.3f   %8.2f MB least, %6.1f GB/s, %5.2f %% of the HBM peak"
                             % (stage, 1e3 * med, 1e3 * min(ts), need[stage] / 1e6, need[stage] / med / 1e9,
                                100.0 * need[stage] / med / HBM_PEAK))
            lines.append("  stage  %-36s %10.3f %10s   %8.2f MB least, %6.1f GB/s, %5.2f %% of the HBM peak"
                         % ("all kernels of a run", 1e3 * total_t, "", total_b / 1e6, total_b / total_t / 1e9,
                            100.0 * total_b / total_t / HBM_PEAK))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
