#!/usr/bin/env python
"""Time global registration (csrc/global_reg.hip) on one MI355X and write profiles/global_reg_timing.txt (or --out).

Clouds: two independent samples of the C1 surface (synthetic.surface, seeds 0 and 1) of n = 10^4 and 10^5 points, the target turned
by rot_zx(140, 65), shifted by (0.7, -1.3, 2.1), noise 0.003; FPFH radii 0.0639 / 0.12 at 10^4, scaled by sqrt(10^4 / n).
Steps per size, each a process of its own under `timeout -k 10` and a kernel trace (rocprofv3 --kernel-trace; --no-trace leaves the
trace out), the whole chain joined with `&&` so that nothing is started after a step that failed:

    features          the descriptors of both clouds (kept in the work directory for the next steps)
    match             nearest_feature (one direction) and feature_matching (both directions and the filter): whole synchronous calls
    ransac H          build, score, best, refine for H = 2^16 and 2^20 on the matches of every source point (mutual = False, so
                      C = n), each between two device synchronisations
    global            the whole registration_global (descriptors, matching, RANSAC with 2^16 hypotheses), mutual = False and True

Kernel times are the trace's (mean and minimum over the launches of a step).  The share of the fp64 vector peak of a sweep is
pairs x fp64 instructions per pair / (39.3e12 lane-instructions per second x kernel time), the MI355X's 78.6 Tflop/s counted with an
FMA as two.  Instructions per pair, from the definition (nothing is fused): matching 3 d = 99 at d = 33 (subtract, multiply, add per
column; the compare and the two selects per pair are left out); scoring 30 = 21 for R p + t - q (9 multiplications, 12 additions), 5
for r^2, the compare, the select, the addition to the sum and the integer addition to the count; its pairs are valid hypotheses x
correspondences (the sweep runs over the compacted valid hypotheses).  --cpu adds the restatement's time (tests/oracle_global_reg.py) at 10^4 on the host."""
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
INSTR_SCORE = 30
SHIFT = np.array([0.7, -1.3, 2.1])
TAU = 0.08
HYPS = (1 << 16, 1 << 20)


def clouds(n):
    from probreg_amd import synthetic

    rot = synthetic.rot_zx(140.0, 65.0)
    src = synthetic.surface(n, 0)
    tgt = synthetic.surface(n, 1) @ rot.T + SHIFT + np.random.default_rng(2).normal(0.0, 0.003, (n, 3))
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), rot


def radii(n):
    s = (1.0e4 / n) ** 0.5
    return 0.0639 * s, 0.12 * s


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


def worker(step, n, work, rounds):
    import torch

    from probreg_amd import _lib, fpfh, global_reg

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    res = {"step": step, "n": n}
    feat = os.path.join(work, "features_%d.npz" % n)
    if step == "features":
        src, tgt, _ = clouds(n)
        fn = fpfh.FPFH(*radii(n))
        (fa, fb), ts = timed(lambda: (fn(src), fn(tgt)), rounds, sync)
        np.savez(feat, fa=fa, fb=fb)
        res["calls"] = {"FPFH of both clouds": ts}
    elif step == "match":
        z = np.load(feat)
        fa, fb = z["fa"], z["fb"]
        _, t1 = timed(lambda: global_reg.nearest_feature(fa, fb), rounds, sync)
        (pairs, _), t2 = timed(lambda: global_reg.feature_matching(fa, fb, mutual=True), rounds, sync)
        every, _ = global_reg.feature_matching(fa, fb, mutual=False)
        np.save(os.path.join(work, "pairs_%d.npy" % n), every)
        res["calls"] = {"nearest_feature (one direction)": t1, "feature_matching (mutual)": t2}
        res["d"] = int(fa.shape[1])
        res["C_mutual"] = int(pairs.shape[0])
    elif step.startswith("ransac"):
        n_hyp = int(step.split(":")[1])
        src, tgt, rot = clouds(n)
        pairs = np.load(os.path.join(work, "pairs_%d.npy" % n))
        plan = global_reg.RansacPlan()
        plan.set_correspondences(src[pairs[:, 0]], tgt[pairs[:, 1]])
        _, tb = timed(lambda: plan.build(0, n_hyp), rounds, sync)
        _, ts = timed(lambda: plan.score(TAU), rounds, sync)
        best, tw = timed(plan.best, rounds, sync)
        (pose, cnt, _, _), tr = timed(lambda: plan.refine(best[3], TAU, 3), rounds, sync)
        _, _, valid = plan.hypotheses(triples=False)
        plan.close()
        c = np.clip((np.trace(rot.T @ pose[:9].reshape(3, 3)) - 1.0) / 2.0, -1.0, 1.0)
        res.update(H=n_hyp, C=int(pairs.shape[0]), valid=int(valid.sum()), inliers=cnt,
                   rot_err_deg=float(np.degrees(np.arccos(c))), t_err=float(np.linalg.norm(pose[9:] - SHIFT)))
        res["calls"] = {"build": tb, "score": ts, "best": tw, "refine (3 refits)": tr}
    elif step == "global":
        src, tgt, rot = clouds(n)
        fn = fpfh.FPFH(*radii(n))
        res["calls"] = {}
        for mutual in (False, True):
            tag = "mutual" if mutual else "every"
            try:
                out, ts = timed(lambda: global_reg.registration_global(src, tgt, feature_fn=fn, max_distance=TAU, mutual=mutual,
                                                                       n_hypotheses=HYPS[0]), rounds, sync)
            except (ValueError, _lib.ProbregHipError) as e:  # too few mutual matches, or none of the draws valid
                res["error_" + tag] = str(e)[:120]
                continue
            c = np.clip((np.trace(rot.T @ out.transformation.rot) - 1.0) / 2.0, -1.0, 1.0)
            res.update({"fitness_" + tag: out.fitness, "rot_err_deg_" + tag: float(np.degrees(np.arccos(c))),
                        "t_err_" + tag: float(np.linalg.norm(out.transformation.t - SHIFT))})
            res["calls"]["registration_global (H = 2^16, mutual = %s)" % mutual] = ts
    with open(os.path.join(work, "%s_%d.json" % (step.replace(":", "_"), n)), "w") as f:
        json.dump(res, f)


def kernel_rows(trace_dir):
    """{short kernel name: (calls, mean ns, min ns)} of the rocpd database(s) a traced step left."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, calls, avg, mn in cur.execute("select name, count(*), avg(end-start), min(end-start) from kernels group by name"):
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            out[short] = (calls, avg, mn)
    return out


def cpu_context(lines):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_fpfh
    import oracle_global_reg as og

    n = 10000
    src, tgt, _ = clouds(n)
    t0 = time.perf_counter()
    fa, fb = oracle_fpfh.describe(src, *radii(n))["fpfh"], oracle_fpfh.describe(tgt, *radii(n))["fpfh"]
    t1 = time.perf_counter()
    pairs, _ = og.feature_matching(fa, fb, True)
    t2 = time.perf_counter()
    og.ransac(src[pairs[:, 0]], tgt[pairs[:, 1]], TAU, HYPS[0], 0)
    t3 = time.perf_counter()
    lines.append("NumPy restatement on the host at n = %d (context only): descriptors %.1f s, matching (both directions) %.1f s, "
                 "RANSAC with 2^16 hypotheses on %d mutual matches %.2f s" % (n, t1 - t0, t2 - t1, pairs.shape[0], t3 - t2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_reg_timing.txt"))
    ap.add_argument("--worker")
    ap.add_argument("--n", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.worker, args.n, args.work, args.rounds)
        return
    work = tempfile.mkdtemp(prefix="global_reg_timing_")
    steps = ["features", "match"] + ["ransac:%d" % h for h in HYPS] + ["global"]
    chain = []
    for n in args.sizes:
        for step in steps:
            cmd = ["timeout", "-k", "10", str(args.limit)]
            if not args.no_trace:
                cmd += ["rocprofv3", "--kernel-trace", "-d", os.path.join(work, "trace_%s_%d" % (step.replace(":", "_"), n)),
                        "-o", "t", "--"]
            cmd += [sys.executable, os.path.abspath(__file__), "--worker", step, "--n", str(n), "--work", work,
                    "--rounds", str(args.rounds)]
            chain.append(" ".join(shlex.quote(c) for c in cmd))
    proc = subprocess.run(" && ".join(chain), shell=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    lines = ["# tools/global_reg_timing.py: %d rounds per call after one warm-up; calls on a host clock between device "
             "synchronisations (ms: median, minimum); kernels from a kernel trace of the same step (ms: mean, minimum, launches)"
             % args.rounds,
             "# share of the fp64 vector peak: pairs x instructions per pair / 39.3e12 lane-instructions/s / mean kernel time; "
             "matching 3 d instructions per pair, scoring %d" % INSTR_SCORE]
    if proc.returncode != 0:
        lines.append("# THE CHAIN STOPPED with exit status %d; the steps before it are below.  Last output:" % proc.returncode)
        lines += ["#   " + s for s in proc.stdout.splitlines()[-15:]]
    for n in args.sizes:
        for step in steps:
            path = os.path.join(work, "%s_%d.json" % (step.replace(":", "_"), n))
            if not os.path.isfile(path):
                continue
            res = json.load(open(path))
            head = "n = %d, %s" % (n, step)
            for k in sorted(res):
                if k not in ("step", "n", "calls"):
                    head += ", %s = %s" % (k, ("%.4g" % res[k]) if isinstance(res[k], float) else res[k])
            lines.append(head)
            for name, ts in res["calls"].items():
                lines.append("  call   %-50s %10.3f %10.3f" % (name, 1e3 * float(np.median(ts)), 1e3 * min(ts)))
            kern = kernel_rows(os.path.join(work, "trace_%s_%d" % (step.replace(":", "_"), n)))
            for name, (calls, avg, mn) in sorted(kern.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
                if not (name.startswith("k_") and ("match" in name or "hyp" in name or "refit" in name or "best" in name
                                                   or "score" in name or "mutual" in name or "valid" in name or "tile" in name)):
                    continue
                line = "  kernel %-50s %10.3f %10.3f %6d" % (name, avg / 1e6, mn / 1e6, calls)
                if name.startswith("k_feature_match") and step == "match":
                    # both directions sweep n x n pairs
                    line += "   %5.1f %% of the fp64 vector peak" % (100.0 * float(n) * n * 3 * res["d"] / LANE_RATE / (avg / 1e9))
                if name == "k_hyp_score" and "H" in res:
                    launches = max(1, (res["valid"] + 65535) // 65536)
                    per = avg / 1e9 * launches  # the launches of one score() together
                    line += "   %5.1f %% of the fp64 vector peak (%d launches per call)" % (
                        100.0 * res["valid"] * float(res["C"]) * INSTR_SCORE / LANE_RATE / per, launches)
                lines.append(line)
    if args.cpu:
        cpu_context(lines)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
