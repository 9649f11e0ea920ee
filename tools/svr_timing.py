#!/usr/bin/env python
"""Time of the SVR feature fit (``svm.OneClassSVM``) and of a whole rigid ``registration_svr`` on one GPU.

    python tools/svr_timing.py [--repeats 5] [--sizes 10000 100000] [--multiples 1 100] [--out profiles/svr_timing.txt]
    python tools/svr_timing.py --sklearn [--sizes 10000 100000]     # the CPU baseline, where scikit-learn is installed

Clouds are ``synthetic.surface(n, 0)``, nu = 0.1, gamma = 1 / (2 sigma^2) and 100 / (2 sigma^2) with sigma the driver's
estimate, tol = 1e-3.  One untimed warm-up solve, then ``--repeats`` timed ones on the same cloud (a solve ends with a
stream synchronisation, so host wall-clock brackets it); median, minimum and maximum are printed.  A further solve with
the library's profile switch on gives device milliseconds per stage (events around every launch, summed over the
rounds): the initial gradient (a pair sweep of n x nu n), the working-set selection, the subproblem (one workgroup) and
the gradient sweep (the q x n pair sweep that computes the kernel rows and consumes them at once, so "row computation"
and "gradient update" are one figure).  The sweep's rate is given in pairs/s; DESIGN.md section 3.8 counts the sweep's 29 fp64
instructions (38 flop) per pair, from which the share of the fp64 vector peak is pairs/s * 38 / 78.6e12.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from probreg_amd import synthetic  # noqa: E402

NU = 0.1
TOL = 1.0e-3
MULTIPLES = (1.0, 100.0)


def sigma_of(x):
    c = x - x.mean(axis=0)
    return float(np.power(np.linalg.det(c.T @ c / (x.shape[0] - 1)), 1.0 / (2.0 * x.shape[1])))


def stats(v):
    v = np.asarray(v) * 1e3
    return "%9.2f ms (min %9.2f, max %9.2f)" % (np.median(v), v.min(), v.max())


def time_fit(n, multiple, repeats, max_iter, emit):
    from probreg_amd import svm

    x = synthetic.surface(n, 0)
    gamma = multiple / (2.0 * sigma_of(x) ** 2)
    q = svm.working_set_size()
    times, info = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        plan = svm.OcsvmPlan()
        plan.set_data(x)
        res = plan.solve(gamma, NU, TOL, max_iter=max_iter)
        alpha, rho, obj, support = plan.solution()
        dt = time.perf_counter() - t0
        plan.close()
        if rep == 0:
            info = (res, obj, support.size)
            continue
        assert (res, obj, support.size) == info  # the solve is byte-repeatable
        times.append(dt)
    (rounds, steps, conv, gap), obj, n_sv = info
    emit("OneClassSVM.compute on surface(%d, 0), gamma = %g / (2 sigma^2) = %.4g, nu = %g, tol = %g: %d rounds of q = %d, "
         "%d SMO steps, converged=%s, gap %.3e, %d support vectors, objective %.9g"
         % (n, multiple, gamma, NU, TOL, rounds, q, steps, conv, gap, n_sv, obj))
    emit("  total    %s" % stats(times))
    plan = svm.OcsvmPlan()
    plan.set_data(x)
    plan.set_profile(True)
    plan.solve(gamma, NU, TOL, max_iter=max_iter)
    ms = plan.profile()
    plan.close()
    emit("  device time by stage: initial gradient %.2f ms, selection %.2f ms, subproblem %.2f ms, gradient sweep %.2f ms"
         % tuple(ms))
    if rounds:
        emit("  per round: selection %.1f us, subproblem %.1f us (%.2f us per SMO step, %.1f steps), sweep %.1f us "
             "(%.3g pairs/s)" % (ms[1] * 1e3 / (rounds + 1), ms[2] * 1e3 / (rounds + 1), ms[2] * 1e3 / max(steps, 1),
                                 steps / rounds, ms[3] * 1e3 / rounds, rounds * q * float(n) / (ms[3] * 1e-3)))
    n_start = min(int(NU * n) + 1, n)
    emit("  initial gradient: %.3g pairs/s" % (float(n) * n_start / (ms[0] * 1e-3)))


def time_registration(n, repeats, emit):
    from probreg_amd import l2dist_regs

    src = synthetic.surface(n, 0)
    rot = synthetic.rot_zx(15.0, 10.0)
    tgt = src @ rot.T
    times, err = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        res = l2dist_regs.registration_svr(src, tgt)
        dt = time.perf_counter() - t0
        err = (float(np.max(np.abs(res.rot - rot))), float(np.max(np.abs(res.t))))
        if rep:
            times.append(dt)
    emit("registration_svr(rigid) on surface(%d, 0): rot_err %.2e, t_err %.2e" % (n, err[0], err[1]))
    emit("  total    %s" % stats(times))


def time_sklearn(sizes, emit):
    from sklearn.svm import OneClassSVM

    for n in sizes:
        x = synthetic.surface(n, 0)
        for multiple in MULTIPLES:
            gamma = multiple / (2.0 * sigma_of(x) ** 2)
            t0 = time.perf_counter()
            clf = OneClassSVM(kernel="rbf", gamma=gamma, nu=NU, tol=TOL, cache_size=4000).fit(x)
            emit("sklearn OneClassSVM(rbf, gamma = %g / (2 sigma^2), nu = %g, tol = %g, cache 4000 MB).fit on "
                 "surface(%d, 0), one CPU thread (libsvm has no others): %.2f s, %d SMO steps, %d support vectors"
                 % (multiple, NU, TOL, n, time.perf_counter() - t0, int(np.ravel(clf.n_iter_)[0]), len(clf.support_)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 5])
    ap.add_argument("--multiples", type=float, nargs="+", default=list(MULTIPLES), help="gamma as multiples of 1 / (2 sigma^2)")
    ap.add_argument("--registration", type=int, default=10 ** 5, help="cloud size of the whole registration (0: skip)")
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sklearn", action="store_true")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    if args.sklearn:
        time_sklearn(args.sizes, emit)
    else:
        for n in args.sizes:
            for multiple in args.multiples:
                time_fit(n, multiple, args.repeats, args.max_iter, emit)
        if args.registration:
            time_registration(args.registration, max(args.repeats // 2, 2), emit)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
