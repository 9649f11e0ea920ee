#!/usr/bin/env python
"""Time of the FPFH descriptor (``fpfh.FPFH``) by stage and of a FilterReg registration on its features, on one GPU.

    python tools/fpfh_timing.py [--repeats 5] [--sizes 10000 100000] [--out profiles/fpfh_timing.txt]
    python tools/fpfh_timing.py --restatement [--sizes 10000]       # the NumPy / SciPy restatement on the CPU, for scale

Clouds are ``synthetic.surface(n, 0)``.  The radii are the median distance to the 30th and to the 100th nearest
neighbour of 2000 sample points (scipy's kd-tree), so the normal search returns about 30 and the feature search about
100 entries and roughly half of the lists are cut by ``max_nn``.  One untimed warm-up, then ``--repeats`` timed runs;
every stage ends with a stream synchronisation, so host wall-clock brackets it.  Median, minimum and maximum are printed,
and per stage the bytes its lists and rows amount to (read + written once) with the rate that gives - the least traffic
the stage could do, not a counter reading.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from probreg_amd import synthetic  # noqa: E402

STAGES = ("upload", "search (normals)", "normals", "search (features)", "spfh", "fpfh", "read-back")


def radii_of(x, ks=(30, 100), sample=2000):
    from scipy.spatial import cKDTree

    q = x[np.random.default_rng(0).choice(x.shape[0], min(sample, x.shape[0]), replace=False)]
    d, _ = cKDTree(x).query(q, k=list(ks))
    return [float(np.median(d[:, i])) for i in range(len(ks))]


def stats(v):
    v = np.asarray(v) * 1e3
    return "%9.3f ms (min %9.3f, max %9.3f)" % (np.median(v), v.min(), v.max())


def staged(fp, x, rn, rf):
    t = [time.perf_counter()]
    plan = fp.FpfhPlan()
    plan.set_data(x)
    t.append(time.perf_counter())
    plan.search(fp.SEARCH_NORMALS, rn, 30)
    t.append(time.perf_counter())
    plan.compute_normals()
    t.append(time.perf_counter())
    plan.search(fp.SEARCH_FEATURES, rf, 100)
    t.append(time.perf_counter())
    plan.compute_spfh()
    t.append(time.perf_counter())
    plan.compute_fpfh()
    t.append(time.perf_counter())
    out = plan.fpfh()
    t.append(time.perf_counter())
    counts = (plan.neighbours(fp.SEARCH_NORMALS)[2], plan.neighbours(fp.SEARCH_FEATURES)[2])
    plan.close()
    return np.diff(t), out, counts


def time_compute(n, repeats, emit):
    from probreg_amd import fpfh as fp

    x = synthetic.surface(n, 0)
    rn, rf = radii_of(x)
    rows, first, counts = [], None, None
    for rep in range(repeats + 1):
        dt, out, counts = staged(fp, x, rn, rf)
        if rep == 0:
            first = out
            continue
        assert out.tobytes() == first.tobytes()  # byte-repeatable
        rows.append(dt)
    rows = np.array(rows)
    cn, cf = counts
    emit("FPFH stages on surface(%d, 0), radius_normal %.4g (lists: mean %.1f, %d of %d cut at 30), radius_feature %.4g "
         "(mean %.1f, %d cut at 100)" % (n, rn, cn.mean(), int((cn == 30).sum()), n, rf, cf.mean(), int((cf == 100).sum())))
    ln, lf = float(cn.sum()), float(cf.sum())
    least = {  # bytes: the lists as stored (idx 4 + d2 8 per slot), a point 32, a normal 24, a row 264
        "search (normals)": n * 32.0 + n * 30 * 12.0, "normals": ln * (4 + 32) + n * 24.0,
        "search (features)": n * 32.0 + n * 100 * 12.0, "spfh": lf * (4 + 32 + 24) + n * 264.0,
        "fpfh": lf * (12 + 264) + n * 264.0}
    for i, name in enumerate(STAGES):
        extra = ""
        if name in least:
            extra = "   least traffic %.1f MB -> %.1f GB/s" % (least[name] / 1e6, least[name] / np.median(rows[:, i]) / 1e9)
        emit("  %-18s %s%s" % (name, stats(rows[:, i]), extra))
    emit("  %-18s %s" % ("sum of stages", stats(rows.sum(axis=1))))
    f = fp.FPFH(rn, rf)
    f.compute(x)
    times = []
    for rep in range(repeats):
        t0 = time.perf_counter()
        f.compute(x)
        times.append(time.perf_counter() - t0)
    emit("  %-18s %s" % ("FPFH.compute", stats(times)))


def time_registration(n, repeats, emit):
    from probreg_amd import filterreg
    from probreg_amd import fpfh as fp

    src, tgt, (rot, t) = synthetic.filterreg_pair(n)
    rn, rf = radii_of(src)
    times, res = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        res = filterreg.registration_filterreg(src, tgt, sigma2=1000, maxiter=5, tol=-1, feature_fn=fp.FPFH(rn, rf))
        if rep:
            times.append(time.perf_counter() - t0)
    emit("registration_filterreg(feature_fn=FPFH(%.4g, %.4g), sigma2=1000, maxiter=5) on filterreg_pair(%d): "
         "6 descriptor evaluations, q %s" % (rn, rf, n, res.q))
    emit("  total              %s" % stats(times))


def time_restatement(sizes, emit):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_fpfh

    for n in sizes:
        x = synthetic.surface(n, 0)
        rn, rf = radii_of(x)
        t0 = time.perf_counter()
        oracle_fpfh.describe(x, rn, rf)
        emit("NumPy / SciPy restatement (tests/oracle_fpfh.py, with its fragility report) on surface(%d, 0), radii %.4g / "
             "%.4g, on the CPU: %.2f s" % (n, rn, rf, time.perf_counter() - t0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 5])
    ap.add_argument("--registration", type=int, default=10 ** 4, help="cloud size of the registration (0: skip)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--restatement", action="store_true")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.restatement:
        time_restatement(args.sizes, emit)
    else:
        for n in args.sizes:
            time_compute(n, args.repeats, emit)
        if args.registration:
            time_registration(args.registration, max(args.repeats // 2, 2), emit)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
