#!/usr/bin/env python
"""Time of the GMMReg feature fit (``features.GMM``) and of a whole ``registration_gmmreg`` on one GPU.

    python tools/time_gmmreg.py [--repeats 7] [--out profiles/gmmreg_timing.txt]
    python tools/time_gmmreg.py --sklearn [--threads 16]      # the CPU baseline, where scikit-learn is installed

Per (N, K) the fit is split into its stages - k-means++ seeding, Lloyd, EM (every entry point ends with a stream
synchronisation, so host wall-clock brackets each stage) - with the Lloyd / EM iteration counts.  One untimed warm-up
run, then ``--repeats`` timed runs on the same cloud; median, minimum and maximum are printed.  Upload of the cloud is
part of ``total`` (what ``GMM.compute`` costs a caller) but of no stage.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from probreg_amd import synthetic  # noqa: E402

FITS = [(10 ** 4, 200), (10 ** 5, 800), (10 ** 6, 800)]


def cloud(n):
    x = synthetic.surface(n, 3)
    return x - x.mean(axis=0)


def stats(v):
    v = np.asarray(v) * 1e3
    return "%9.2f ms (min %9.2f, max %9.2f)" % (np.median(v), v.min(), v.max())


def time_fit(x, k, repeats, emit):
    from probreg_amd import features

    rows = {key: [] for key in ("seeding", "lloyd", "em", "total")}
    info = None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        plan = features.GmmFitPlan()
        plan.set_data(x)
        t1 = time.perf_counter()
        plan.seed(k, features.seed_uniforms(k, 0))
        t2 = time.perf_counter()
        n_lloyd = plan.lloyd(features.LLOYD_MAX_ITER, features.lloyd_tolerance(x))
        plan.init_from_labels(1.0e-6)
        t3 = time.perf_counter()
        n_em, conv, lbs = plan.em(1.0e-3, 100, 1.0e-6)
        plan.params()
        t4 = time.perf_counter()
        plan.close()
        if rep == 0:
            info = (n_lloyd, n_em, conv, lbs[-1])
            continue
        assert (n_lloyd, n_em, conv, lbs[-1]) == info  # the fit is byte-repeatable
        for key, dt in zip(("seeding", "lloyd", "em", "total"), (t2 - t1, t3 - t2, t4 - t3, t4 - t0)):
            rows[key].append(dt)
    emit("GMM(%d).compute on surface(%d): %d Lloyd + %d EM iterations, converged=%s, lower bound %.5f"
         % (k, x.shape[0], info[0], info[1], info[2], info[3]))
    for key in ("seeding", "lloyd", "em", "total"):
        emit("  %-8s %s" % (key, stats(rows[key])))
    emit("  per EM iteration %.3f ms, per Lloyd iteration %.3f ms"
         % (np.median(rows["em"]) * 1e3 / info[1], np.median(rows["lloyd"]) * 1e3 / info[0]))


def time_registration(n, k, repeats, emit):
    from probreg_amd import l2dist_regs

    src = cloud(n)
    rot, t = synthetic.rot_zx(15.0, 10.0), np.array([0.05, -0.03, 0.02])
    tgt = src @ rot.T + t
    times, err = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        res = l2dist_regs.registration_gmmreg(src, tgt, "rigid", n_gmm_components=k)
        dt = time.perf_counter() - t0
        err = (float(np.max(np.abs(res.rot - rot))), float(np.max(np.abs(res.t - t))))
        if rep:
            times.append(dt)
    emit("registration_gmmreg(rigid) on surface(%d), K = %d: rot_err %.2e, t_err %.2e" % (n, k, err[0], err[1]))
    emit("  total    %s" % stats(times))


def time_sklearn(threads, emit):
    from sklearn.mixture import GaussianMixture

    try:
        from threadpoolctl import threadpool_limits
    except ImportError:  # pragma: no cover
        threadpool_limits = None
    for n, k in FITS[:2]:
        x = cloud(n)
        t0 = time.perf_counter()
        if threadpool_limits is not None:
            with threadpool_limits(limits=threads):
                gm = GaussianMixture(k, covariance_type="spherical", random_state=0).fit(x)
        else:
            gm = GaussianMixture(k, covariance_type="spherical", random_state=0).fit(x)
        emit("sklearn GaussianMixture(%d, spherical).fit on surface(%d), %d CPU threads: %.2f s, %d EM iterations, "
             "lower bound %.5f" % (k, n, threads, time.perf_counter() - t0, gm.n_iter_, gm.lower_bound_))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.sklearn:
        time_sklearn(args.threads, emit)
    else:
        for n, k in FITS:
            time_fit(cloud(n), k, args.repeats, emit)
        time_registration(10 ** 5, 800, max(args.repeats // 2, 2), emit)
    if args.out:
        with open(args.out, "a" if args.sklearn else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
