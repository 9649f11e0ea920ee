#!/usr/bin/env python
"""Time the kernel-field evaluation (csrc/field.hip) on one MI355X and write profiles/field_timing.txt (or --out).

Every kernel function at Q = 10^6 queries on M = 10^4 control points (one slab) and at Q = 10^5 on M = 10^5 (two slabs, whose
sums k_field_add_slabs adds): gaussian (beta 0.05), imq (c 1) and the 3-D spline with D = 3, C = 3, the 2-D spline with D = 2, C = 2.
Control points and queries are independent samples of synthetic.surface, the weights are standard normal.

    call     KernelField.evaluate from host arrays (upload of the queries, kernels, read-back), host clock between two device
             synchronisations, median and minimum over --rounds after one warm-up
    kernel   k_field (and k_field_add_slabs) alone, summed over the launches of one evaluate, from a kernel trace of a run of its
             own; the share of the fp64 vector peak is pairs x fp64 instructions per pair / 39.3e12 lane-instructions/s / kernel
             time (78.6 Tflop/s with an FMA as two).  The instructions per pair are counted in the gfx950 code of the loop body
             (8 pairs per trip: 4 control points x 2 queries per lane), CASES below; all vector instructions in brackets.
    route    for the gaussian only, the one way to evaluate the field before this kernel existed:
             GaussTransform(control, sqrt(2 beta), exact=True).compute(points, W.T), same run, same inputs (k_gauss_direct_f64,
             one sweep per two weight rows)

One child process for the calls and one under `rocprofv3 --kernel-trace` for the kernel times; each under `timeout -k 10`, and
nothing is started after a child that failed."""
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

LANE_RATE = 39.3e12
SHAPES = ((1000000, 10000), (100000, 100000))
# name -> (kernel, param, D, C, fp64 instructions per pair, all vector instructions per pair)
CASES = {"gaussian": ("gaussian", 0.05, 3, 3, 30.0, 40.1), "imq": ("imq", 1.0, 3, 3, 19.0, 25.9),
         "tps 2-D": ("tps", None, 2, 2, 84.0, 103.0), "tps 3-D": ("tps", None, 3, 3, 23.0, 34.3)}


def inputs(q, m, dim, cols):
    from probreg_amd import synthetic

    rng = np.random.default_rng(q + m)
    return (np.ascontiguousarray(synthetic.surface(m, 1)[:, :dim]), rng.normal(size=(m, cols)),
            np.ascontiguousarray(synthetic.surface(q, 2)[:, :dim]))


def clock(fn, rounds, sync):
    ts = []
    for _ in range(rounds + 1):  # the first one warms up
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return ts[1:]


def worker(work, mode, rounds):
    import torch

    from probreg_amd import _lib
    from probreg_amd.field import KernelField
    from probreg_amd.gauss_transform import GaussTransform

    _lib.require_gpu()
    sync = torch.cuda.synchronize
    res = {}
    for q, m in SHAPES:
        for name, (kernel, param, dim, cols, _, _) in CASES.items():
            control, w, points = inputs(q, m, dim, cols)
            field = KernelField(control, w, kernel, param)
            try:
                res["%s/%d/%d" % (name, q, m)] = clock(lambda: field.evaluate(points), rounds, sync)
                if kernel == "gaussian":
                    route = GaussTransform(control, np.sqrt(2.0 * param), exact=True)
                    wt = np.ascontiguousarray(w.T)
                    res["route/%d/%d" % (q, m)] = clock(lambda: route.compute(points, wt), rounds, sync)
                    res["route_diff/%d/%d" % (q, m)] = float(np.abs(route.compute(points, wt).T - field.evaluate(points)).max())
            finally:
                field.close()
    with open(os.path.join(work, mode + ".json"), "w") as f:
        json.dump(res, f)


KIND_OF = {"gaussian": 0, "imq": 1, "tps 2-D": 2, "tps 3-D": 3}  # the first template argument of k_field


def traced(trace_dir):
    """name -> seconds of every launch, in launch order; an instance of k_field is named k_field/<kind>/<C>."""
    out = {}
    for db in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        cur = sqlite3.connect(db).cursor()
        for name, start, end in cur.execute("select name, start, end from kernels order by start"):
            inst = re.search(r"k_field<\s*(\d+),\s*(\d+)>", name) or re.search(r"k_fieldILi(\d+)ELi(\d+)E", name)
            if inst:
                key = "k_field/%s/%s" % inst.groups()
            else:
                key = next((k for k in ("k_field_add_slabs", "k_gauss_direct_f64") if k in name), None)
            if key:
                out.setdefault(key, []).append((end - start) * 1.0e-9)
    return out


def batches_of(q, m, cols):
    """The launches of k_field per evaluate (prg_field_evaluate: one slab: one; else batches that keep the slab sums in 64 MB)."""
    slabs = -(-(-(-m // 4) * 4) // 65536)
    if slabs == 1:
        return 1
    return -(-q // min(max((64 << 20) // (8 * cols * slabs) // 128, 1) * 128, q))


def per_call(launches, rounds):
    """{case/q/m: [kernel seconds per evaluate]} from the launches of the worker, which come per shape and case as rounds + 1
    evaluates (the first a warm-up), for the gaussian then rounds + 2 calls of the older route and one more evaluate.  None
    when the trace does not hold exactly those launches."""
    out, used = {}, {}

    def take(key, count):
        first = used.get(key, 0)
        used[key] = first + count
        got = launches.get(key, [])[first:first + count]
        return got if len(got) == count else None

    for q, m in SHAPES:
        for name, (kernel, _, _, cols, _, _) in CASES.items():
            evals = rounds + 1 + (kernel == "gaussian")
            nb = batches_of(q, m, cols)
            main_k = take("k_field/%d/%d" % (KIND_OF[name], cols), evals * nb)
            adds = take("k_field_add_slabs", evals * nb) if m > 65536 else [0.0] * (evals * nb)
            if main_k is None or adds is None:
                return None
            per = [sum(main_k[e * nb:(e + 1) * nb]) + sum(adds[e * nb:(e + 1) * nb]) for e in range(evals)]
            out["%s/%d/%d" % (name, q, m)] = per[1:rounds + 1]
            if kernel == "gaussian":
                sweeps = take("k_gauss_direct_f64", 2 * (rounds + 2))  # C = 3: a sweep of two weight rows, then one of one
                if sweeps is None:
                    return None
                out["route/%d/%d" % (q, m)] = [sweeps[2 * e] + sweeps[2 * e + 1] for e in range(1, rounds + 1)]
    if any(used[k] != len(launches.get(k, [])) for k in used):
        return None
    return out


def ms(ts):
    return "%10.3f %10.3f" % (1e3 * float(np.median(ts)), 1e3 * min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_timing.txt"))
    ap.add_argument("--worker")
    ap.add_argument("--work")
    args = ap.parse_args()
    if args.worker:
        worker(args.work, args.worker, args.rounds)
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    work = tempfile.mkdtemp(prefix="field_timing_")
    lines = ["# tools/field_timing.py: KernelField.evaluate, %d rounds after one warm-up; ms: median, minimum" % args.rounds,
             "# call: host clock around evaluate from host arrays (upload, kernels, read-back); kernel: the launches of one "
             "evaluate summed, from a kernel trace of a run of its own",
             "# share of the fp64 vector peak: pairs x fp64 instructions per pair / 39.3e12 lane-instructions/s / median "
             "kernel time; instructions per pair counted in the gfx950 loop body (all vector instructions in brackets)"]
    failed = False

    def child(mode, trace=None):
        cmd = ["timeout", "-k", "10", str(args.limit)]
        if trace:
            cmd += ["rocprofv3", "--kernel-trace", "-d", trace, "-o", "t", "--"]
        cmd += [sys.executable, os.path.abspath(__file__), "--worker", mode, "--work", work, "--rounds", str(args.rounds)]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        if proc.returncode != 0:  # nothing is started on the device after a step that failed
            lines.append("# STOPPED: %s ended with exit status %d.  Last output:" % (mode, proc.returncode))
            lines.extend("#   " + s for s in proc.stdout.splitlines()[-15:])
            return False
        return True

    calls = kernels = None
    if child("calls"):
        calls = json.load(open(os.path.join(work, "calls.json")))
        trace = os.path.join(work, "trace")
        if child("kernels", trace):
            launches = traced(trace)
            kernels = per_call(launches, args.rounds)
            if kernels is None:
                lines.append("# the kernel trace does not hold the launches of the worker: " + ", ".join(
                    "%s x %d" % (k, len(v)) for k, v in sorted(launches.items())))
        else:
            failed = True
    else:
        failed = True
    if calls:
        for q, m in SHAPES:
            lines.append("Q = %d queries, M = %d control points (%d slab%s), %.3g pairs" % (q, m, -(-m // 65536),
                                                                                       "" if m <= 65536 else "s", float(q) * m))
            for name, (kernel, param, dim, cols, f64, valu) in CASES.items():
                key = "%s/%d/%d" % (name, q, m)
                lines.append("  call    %-46s %s" % ("%s, D = %d, C = %d" % (name, dim, cols), ms(calls[key])))
                if kernels and kernels.get(key) and min(kernels[key]) > 0.0:
                    share = float(q) * m * f64 / LANE_RATE / float(np.median(kernels[key]))
                    lines.append("  kernel  %-46s %s   %4.1f (%5.1f) instructions per pair, %5.1f %% of the fp64 vector peak"
                                 % ("k_field" + (" + k_field_add_slabs" if m > 65536 else ""), ms(kernels[key]), f64, valu,
                                    100.0 * share))
                if kernel == "gaussian":
                    rkey = "route/%d/%d" % (q, m)
                    lines.append("  call    %-46s %s   (largest difference from the field: %.3g)"
                                 % ("route: GaussTransform(exact=True).compute", ms(calls[rkey]), calls["route_diff/%d/%d" % (q, m)]))
                    if kernels and kernels.get(rkey) and min(kernels[rkey]) > 0.0:
                        lines.append("  kernel  %-46s %s" % ("route: k_gauss_direct_f64<2> + <1>", ms(kernels[rkey])))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    if failed:
        sys.exit(1)


if __name__ == "__main__":
    main()
