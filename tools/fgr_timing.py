#!/usr/bin/env python
"""Time fast global registration (csrc/fgr.hip) on one MI355X and write profiles/fgr_timing.txt (or --out).

Input per size C = 10^3 .. 10^6: the C1 surface with C points, the same points turned by rot_zx(140, 65), shifted and with
noise 0.002 as the target, and C correspondences of which 70 % have a random partner.

Steps per C, each a process of its own under `timeout -k 10`, the whole chain joined with `&&` so that nothing is started
after a step that failed.  Every step runs twice: once plain, for the call times (a host clock between two device
synchronisations: median and minimum over the rounds after one warm-up), and once under a kernel trace (rocprofv3
--kernel-trace), for the kernel times (mean and minimum over the launches); the traced run's call times are not reported.

    tuples                        FgrPlan.tuples (cap 1000): the trial kernel, the ordered compaction, the gather
    sums / one iteration / loop   on the K <= 3000 used pairs of the tuple test, and on all K = C pairs without it
    registration_fgr              the whole call from host arrays, with and without the tuple test
    registration_ransac           65 536 hypotheses on the same correspondences, in the same run

The sums kernel reads 48 bytes per used pair; its bandwidth is K x 48 B / kernel time against the HBM peak of 8 TB/s.
--cpu adds the NumPy restatement's time (tests/oracle_fgr.py) on the host at the sizes it can do."""
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

HBM_PEAK = 8.0e12
PAIR_BYTES = 48
WRONG, NOISE, TAU, N_HYP = 0.7, 0.002, 0.02, 65536
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


def case(c):
    from probreg_amd import synthetic

    rng = np.random.default_rng(c)
    src = np.ascontiguousarray(synthetic.surface(c, 7))
    tgt = np.ascontiguousarray(src @ synthetic.rot_zx(140.0, 65.0).T + np.array([0.7, -1.3, 2.1]) + rng.normal(0.0, NOISE, src.shape))
    i = rng.permutation(c)
    j = i.copy()
    bad = rng.permutation(c)[:int(WRONG * c)]
    j[bad] = (i[bad] + rng.integers(1, c, bad.shape[0])) % c
    return src, tgt, np.stack([i, j], axis=1).astype(np.int32)


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


def worker(c, work, rounds, tag):
    import torch

    from probreg_amd import _lib, global_reg as gr

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    src, tgt, corr = case(c)
    plan = gr.FgrPlan()
    plan.set_clouds(src, tgt)
    plan.set_correspondences(corr)
    _, tn = timed(plan.normalise, rounds, sync)
    tup, tt = timed(lambda: plan.tuples(0), rounds, sync)
    calls = {"normalise": tn, "tuples (cap 1000)": tt}

    def loop(n):
        plan.set_state(IDENTITY, 1.0)
        return plan.iterate(n)

    for label in ("K = %d (tuple test)" % tup[0].shape[0], "K = C = %d (no tuple test)" % c):
        if label.startswith("K = C"):
            plan.set_used(np.arange(c, dtype=np.int32))
        plan.set_state(IDENTITY, 1.0)
        _, t1 = timed(plan.sums, rounds, sync)
        _, t2 = timed(lambda: loop(1), rounds, sync)
        _, t3 = timed(lambda: loop(64), rounds, sync)
        calls["sums, " + label] = t1
        calls["one iteration (set_state, sums, step, state), " + label] = t2
        calls["64-iteration loop (set_state, iterate, state), " + label] = t3
    plan.close()
    res = {"C": c, "n_tuples": tup[1], "n_trials": tup[2]}
    if tag == "plain":  # the whole calls stay out of the traced run, whose kernels are then those of the stages alone
        a, ta = timed(lambda: gr.registration_fgr(src, tgt, corr, max_distance=TAU), rounds, sync)
        b, tb = timed(lambda: gr.registration_fgr(src, tgt, corr, max_distance=TAU, tuple_test=False), rounds, sync)
        r, tr = timed(lambda: gr.registration_ransac(src, tgt, corr, TAU, n_hypotheses=N_HYP), rounds, sync)
        calls["registration_fgr (whole call, tuple test)"] = ta
        calls["registration_fgr (whole call, no tuple test)"] = tb
        calls["registration_ransac (whole call, %d hypotheses)" % N_HYP] = tr
        res.update(fitness=[a.fitness, b.fitness, r.fitness], status=[a.status, b.status])
    res["calls"] = calls
    with open(os.path.join(work, "%s_%d.json" % (tag, c)), "w") as f:
        json.dump(res, f)
    print("fgr_timing: %s run of C = %d done" % (tag, c), flush=True)


def kernel_rows(trace_dir):
    """{short kernel name: (calls, mean ns, min ns, max ns)} of the rocpd database(s) a traced step left."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, calls, avg, mn, mx in cur.execute(
                "select name, count(*), avg(end-start), min(end-start), max(end-start) from kernels group by name"):
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            out[short] = (calls, avg, mn, mx)
    return out


def cpu_context(lines, sizes):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_fgr as of

    for c in sizes:
        src, tgt, corr = case(c)
        for tuple_test in (True, False):
            t0 = time.perf_counter()
            r = of.fgr(src, tgt, corr, tuple_test=tuple_test)
            lines.append("NumPy restatement on the host (context only): C = %d, tuple test %s: %.2f s (%d used pairs, status %s)"
                         % (c, tuple_test, time.perf_counter() - t0, r["used"].shape[0], r["status"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000, 1000000])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--limit", type=int, default=150, help="seconds a step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fgr_timing.txt"))
    ap.add_argument("--worker")
    ap.add_argument("--c", type=int)
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.c, args.work, args.rounds, args.worker)
        return
    work = tempfile.mkdtemp(prefix="fgr_timing_")
    chain = []
    for c in args.sizes:
        for tag in ("plain",) if args.no_trace else ("plain", "traced"):
            cmd = ["timeout", "-k", "10", str(args.limit)]
            if tag == "traced":
                cmd += ["rocprofv3", "--kernel-trace", "-d", os.path.join(work, "trace_%d" % c), "-o", "t", "--"]
            cmd += [sys.executable, os.path.abspath(__file__), "--worker", tag, "--c", str(c), "--work", work,
                    "--rounds", str(args.rounds)]
            chain.append(" ".join(shlex.quote(x) for x in cmd))
    proc = subprocess.run(" && ".join(chain), shell=True)  # the steps' own lines go straight through, as progress
    lines = ["# tools/fgr_timing.py: %d rounds per call after one warm-up; calls on a host clock between device synchronisations, "
             "in a run without a profiler (ms: median, minimum); kernels from a kernel trace of a second run of the same step "
             "(ms: mean, minimum, maximum, launches)" % args.rounds,
             "# k_fgr_sums runs on K <= 3000 pairs (its minimum) and on K = C pairs (its maximum): bandwidth = C x %d B / maximum, "
             "against %.0f TB/s" % (PAIR_BYTES, HBM_PEAK / 1e12)]
    if proc.returncode != 0:
        lines.append("# THE CHAIN STOPPED with exit status %d; the steps before it are below." % proc.returncode)
    for c in args.sizes:
        path = os.path.join(work, "plain_%d.json" % c)
        if not os.path.isfile(path):
            continue
        res = json.load(open(path))
        lines.append("C = %d, %d tuples in %d trials, fitness (fgr, fgr without the tuple test, ransac) = %s, status = %s"
                     % (c, res["n_tuples"], res["n_trials"], ["%.3f" % v for v in res["fitness"]], res["status"]))
        for name, ts in res["calls"].items():
            lines.append("  call   %-72s %10.3f %10.3f" % (name, 1e3 * float(np.median(ts)), 1e3 * min(ts)))
        kern = kernel_rows(os.path.join(work, "trace_%d" % c))
        for name, (calls, avg, mn, mx) in sorted(kern.items(), key=lambda kv: -kv[1][0] * kv[1][1]):
            if not name.startswith("k_fgr"):
                continue
            line = "  kernel %-30s %10.4f %10.4f %10.4f %6d" % (name, avg / 1e6, mn / 1e6, mx / 1e6, calls)
            if name == "k_fgr_sums":
                line += "   K = C: %.1f GB/s, %.2f %% of the HBM peak" % (c * PAIR_BYTES / (mx / 1e9) / 1e9,
                                                                      100.0 * c * PAIR_BYTES / (mx / 1e9) / HBM_PEAK)
            lines.append(line)
    text = "\n".join(lines) + "\n"
    if args.cpu:
        extra = []
        cpu_context(extra, [1000, 10000])
        text += "\n".join(extra) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
