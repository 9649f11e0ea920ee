#!/usr/bin/env python
"""Time plane segmentation (csrc/plane_seg.hip) on one MI355X and write profiles/plane_timing.txt (or --out).

Clouds: the table scene of the tests scaled to n = 10^4, 10^5 and 10^6 points (two thirds on a table top tilted by
rot_zx(25, 12) with uniform noise +-0.004, the C1 surface twice as objects above it, 4 % uniform outliers, all permuted) and,
for segment_planes, the room scene scaled likewise (a floor and two walls).  tau = 0.01, H = 1000 and 65536.

Steps per (n, H), each a process of its own under `timeout -k 10`, the whole chain joined with `&&` so that nothing is started
after a step that failed.  Every step runs twice: once plain, for the call times (a host clock between two device
synchronisations: median and minimum over the rounds after one warm-up), and once under a kernel trace (rocprofv3 --kernel-trace),
for the kernel times (mean and minimum over the launches); the traced run's call times are not reported.

    build, score, best, one refit step     the stages of a PlanePlan that holds the cloud
    segment_plane                          the whole call from host arrays (upload, all stages, 3 refits, results back)
    segment_planes (3 planes)              the whole call on the room scene
    k_hyp_score of global_reg              RansacPlan.score at the same H with C = n correspondences (the cloud and a rigid copy
                                           of it, so that nearly every hypothesis is valid, as here): like with like

The share of the fp64 vector peak of a sweep is pairs x fp64 instructions per pair / (39.3e12 lane-instructions per second x
kernel time), the MI355X's 78.6 Tflop/s counted with an FMA as two.  Instructions per pair, from the definition (nothing is
fused): plane scoring 13 = 3 subtractions, 3 multiplications and 2 additions for the distance, the absolute compare, d d, the
select, the addition to the sum and the integer addition to the count; pose scoring 30 (tools/global_reg_timing.py).  Pairs are
valid hypotheses x points.  --cpu adds the NumPy restatement's time (tests/oracle_plane.py) on the host at the sizes it can do."""
import argparse
import glob
import json
import os
import shlex
import sqlite3
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LANE_RATE = 78.6e12 / 2.0
INSTR_PLANE, INSTR_POSE = 13, 30
TAU = 0.01
NOISE = 0.004
HYPS = (1000, 65536)


def table_scene(n):
    from probreg_amd import synthetic

    rng = np.random.default_rng(n)
    k, n_out = (2 * n) // 3, n // 25
    n1 = (n - k - n_out) * 3 // 5
    n2 = n - k - n_out - n1
    top = np.stack([rng.uniform(-1.0, 1.0, k), rng.uniform(-1.0, 1.0, k), rng.uniform(-NOISE, NOISE, k)], axis=1)
    o1 = 0.5 * synthetic.surface(n1, 11) + np.array([-0.4, 0.3, 0.8])
    o2 = 0.4 * synthetic.surface(n2, 12) + np.array([0.45, -0.35, 0.9])
    out = np.stack([rng.uniform(-1.2, 1.2, n_out), rng.uniform(-1.2, 1.2, n_out), rng.uniform(-0.5, 1.5, n_out)], axis=1)
    pts = np.concatenate([top, o1, o2, out]) @ synthetic.rot_zx(25.0, 12.0).T + np.array([0.3, -0.2, 0.5])
    return np.ascontiguousarray(pts[rng.permutation(n)])


def room_scene(n):
    from probreg_amd import synthetic

    rng = np.random.default_rng(n + 1)
    nf, n1, n2 = n // 2, (3 * n) // 10, n // 6
    n_out = n - nf - n1 - n2
    floor = np.stack([rng.uniform(0.0, 2.0, nf), rng.uniform(0.0, 1.6, nf), rng.uniform(-NOISE, NOISE, nf)], axis=1)
    wall1 = np.stack([rng.uniform(0.0, 2.0, n1), rng.uniform(-NOISE, NOISE, n1), rng.uniform(0.05, 1.2, n1)], axis=1)
    wall2 = np.stack([rng.uniform(-NOISE, NOISE, n2), rng.uniform(0.05, 1.6, n2), rng.uniform(0.05, 1.2, n2)], axis=1)
    out = np.stack([rng.uniform(0.1, 2.0, n_out), rng.uniform(0.1, 1.6, n_out), rng.uniform(0.1, 1.2, n_out)], axis=1)
    pts = np.concatenate([floor, wall1, wall2, out]) @ synthetic.rot_zx(40.0, 20.0).T
    return np.ascontiguousarray(pts[rng.permutation(n)])


def timed(fn, rounds, sync):
    fn()
    sync()
    ts = []
    for _ in range(rounds):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return out, ts


def worker(n, n_hyp, work, rounds, tag):
    import torch

    from probreg_amd import _lib, global_reg, preprocess, synthetic

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    pts = table_scene(n)
    room = room_scene(n) if tag == "plain" else None
    plan = preprocess.PlanePlan()
    plan.set_points(pts)
    _, tb = timed(lambda: plan.build(0, n_hyp), rounds, sync)
    _, ts = timed(lambda: plan.score(TAU), rounds, sync)
    best, tw = timed(plan.best, rounds, sync)
    _, tr = timed(lambda: plan.refine(best[4], TAU, 1), rounds, sync)
    plan.close()
    calls = {"build": tb, "score": ts, "best": tw, "one refit step": tr}
    res = {"n": n, "H": n_hyp, "valid": best[1], "winner_count": best[2]}
    if tag == "plain":  # the whole calls stay out of the traced run, whose sweeps are then those of score() alone
        seg, t1 = timed(lambda: preprocess.segment_plane(pts, TAU, n_hyp), rounds, sync)
        planes, t3 = timed(lambda: preprocess.segment_planes(room, TAU, 3, 100, n_hyp), rounds, sync)
        calls["segment_plane (whole call, 3 refits)"] = t1
        calls["segment_planes (3 planes, room scene)"] = t3
        res.update(inliers=int(seg.inliers.shape[0]), planes=planes.sizes.tolist())
    rot = synthetic.rot_zx(140.0, 65.0)
    rp = global_reg.RansacPlan()
    rp.set_correspondences(pts, pts @ rot.T + np.array([0.7, -1.3, 2.1]))
    rp.build(0, n_hyp)
    _, tp = timed(lambda: rp.score(TAU), rounds, sync)
    _, _, pose_valid = rp.hypotheses(triples=False)
    rp.close()
    calls["RansacPlan.score (global_reg, C = n)"] = tp
    res.update(pose_valid=int(pose_valid.sum()), calls=calls)
    with open(os.path.join(work, "%s_%d_%d.json" % (tag, n, n_hyp)), "w") as f:
        json.dump(res, f)
    print("plane_timing: %s run of n = %d, H = %d done" % (tag, n, n_hyp), flush=True)


def kernel_rows(trace_dir):
    """{short kernel name: (calls, mean ns, min ns)} of the rocpd database(s) a traced step left."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, calls, avg, mn in cur.execute("select name, count(*), avg(end-start), min(end-start) from kernels group by name"):
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            out[short] = (calls, avg, mn)
    return out


def cpu_context(lines, sizes):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_plane as op

    for n, n_hyp in sizes:
        pts = table_scene(n)
        t0 = time.perf_counter()
        r = op.segment_plane(pts, TAU, n_hyp)
        lines.append("NumPy restatement on the host (context only): segment_plane at n = %d, H = %d: %.2f s (%d inliers)"
                     % (n, n_hyp, time.perf_counter() - t0, r["inliers"].shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--hyps", type=int, nargs="+", default=list(HYPS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_timing.txt"))
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--h", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.n, args.h, args.work, args.rounds, args.worker)
        return
    work = tempfile.mkdtemp(prefix="plane_timing_")
    configs = [(n, h) for n in args.sizes for h in args.hyps]
    chain = []
    for n, h in configs:
        for tag in ("plain",) if args.no_trace else ("plain", "traced"):
            cmd = ["timeout", "-k", "10", str(args.limit)]
            if tag == "traced":
                cmd += ["rocprofv3", "--kernel-trace", "-d", os.path.join(work, "trace_%d_%d" % (n, h)), "-o", "t", "--"]
            cmd += [sys.executable, os.path.abspath(__file__), "--worker", tag, "--n", str(n), "--h", str(h), "--work", work,
                    "--rounds", str(args.rounds)]
            chain.append(" ".join(shlex.quote(c) for c in cmd))
    proc = subprocess.run(" && ".join(chain), shell=True)  # the steps' own lines go straight through, as progress
    lines = ["# tools/plane_timing.py: %d rounds per call after one warm-up; calls on a host clock between device synchronisations, "
             "in a run without a profiler (ms: median, minimum); kernels from a kernel trace of a second run of the same step "
             "(ms: mean, minimum, launches)" % args.rounds,
             "# share of the fp64 vector peak: valid hypotheses x points x instructions per pair / 39.3e12 lane-instructions/s / "
             "the kernel time of one score(); plane scoring %d instructions per pair, pose scoring %d" % (INSTR_PLANE, INSTR_POSE)]
    if proc.returncode != 0:
        lines.append("# THE CHAIN STOPPED with exit status %d; the steps before it are below." % proc.returncode)
    for n, h in configs:
        path = os.path.join(work, "plain_%d_%d.json" % (n, h))
        if not os.path.isfile(path):
            continue
        res = json.load(open(path))
        lines.append("n = %d, H = %d, valid = %d, winner's count = %d, final inliers = %d, room planes = %s, valid pose hypotheses = %d"
                     % (n, h, res["valid"], res["winner_count"], res["inliers"], res["planes"], res["pose_valid"]))
        for name, ts in res["calls"].items():
            lines.append("  call   %-50s %10.3f %10.3f" % (name, 1e3 * float(np.median(ts)), 1e3 * min(ts)))
        kern = kernel_rows(os.path.join(work, "trace_%d_%d" % (n, h)))
        for name, (calls, avg, mn) in sorted(kern.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            if not name.startswith("k_"):
                continue
            line = "  kernel %-50s %10.3f %10.3f %6d" % (name, avg / 1e6, mn / 1e6, calls)
            per_call = avg / 1e9 * calls / (args.rounds + 1)  # the launches of one score() together
            if name.startswith("k_plane_score"):
                line += "   %5.1f %% of the fp64 vector peak (%d launches per score)" % (
                    100.0 * res["valid"] * float(n) * INSTR_PLANE / LANE_RATE / per_call, calls // (args.rounds + 1))
            if name == "k_hyp_score":
                line += "   %5.1f %% of the fp64 vector peak (%d launches per score)" % (
                    100.0 * res["pose_valid"] * float(n) * INSTR_POSE / LANE_RATE / per_call, calls // (args.rounds + 1))
            lines.append(line)
    text = "\n".join(lines) + "\n"
    if args.cpu:
        extra = []
        cpu_context(extra, [(10000, 1000), (100000, 1000)])
        text += "\n".join(extra) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
