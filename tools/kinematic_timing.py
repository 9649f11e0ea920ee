#!/usr/bin/env python
"""Times of the deformable kinematic FilterReg on one GPU, beside its NumPy restatement.

    python tools/kinematic_timing.py [--m 100000] [--k 16] [--repeats 5] [--out profiles/kinematic_timing.txt]
    python tools/kinematic_timing.py --restatement          # tests/oracle_kinematic.py on the CPU, for scale

The cloud is the clustered bar of tests/kinematic_cases.py with M = N and its motion scaled by 4 / K, so that the last
node moves as far as that of the 4-node test clouds (at the bar's own motion a 16th node turns by 32 degrees, 40 % of the
source finds no target at sigma2 = 1e-3 and the Gauss-Newton loop of the definition diverges, on the CPU as well).  Timed, each ending in a stream synchronisation
(every call reads a result back), after one untimed warm-up: ``DeformableKinematicModel.transform``; one M-step on the
plan's E-step values (normal sums, pseudo-inverse, the Gauss-Newton inner loop; its iteration count is printed); one EM
iteration of the device-resident loop (skinning, lattice E-step, M-step), taken between the callbacks of a registration.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kinematic_cases as kc  # noqa: E402
import oracle_kinematic as ok  # noqa: E402


def stats(v):
    v = np.asarray(v) * 1e3
    return "%10.3f ms (min %10.3f, max %10.3f)" % (np.median(v), v.min(), v.max())


def gpu(case, args, emit):
    from probreg_amd import filterreg as fr
    from probreg_amd import transformation as tf

    weights = tf.DeformableKinematicModel.make_weight(case.pairs, case.vals)
    model = tf.DeformableKinematicModel(case.truth, weights)
    model.transform(case.source)
    t = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        model.transform(case.source)
        t.append(time.perf_counter() - t0)
    emit("  DeformableKinematicModel.transform %s" % stats(t))

    plan = fr._Plan()
    try:
        plan.set_source(case.source)
        plan.set_target(case.target)
        plan.set_skinning(case.pairs, case.vals, case.n_nodes)
        ident = tf.dualquat_identity(case.n_nodes)
        plan.set_dualquats(ident)
        plan.kinematic_estep(args.sigma2)
        fr._kinematic_solve(plan, ident, args.sigma2, 0.0, False, 50, 1e-4, False)
        t, te, inner = [], [], 0
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            plan.kinematic_estep(args.sigma2)
            plan.get_dualquats()  # (a small read-back: the E-step itself is only enqueued)
            t1 = time.perf_counter()
            inner = fr._kinematic_solve(plan, ident, args.sigma2, 0.0, False, 50, 1e-4, False)[3]
            t.append(time.perf_counter() - t1)
            te.append(t1 - t0)
        emit("  skinning + lattice E-step          %s" % stats(te))
        emit("  M-step, %2d inner iterations        %s" % (inner, stats(t)))
        t = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            plan.kinematic_grad_sums(np.zeros(6 * case.n_nodes), False)
            t.append(time.perf_counter() - t0)
        emit("  one gradient pass                  %s" % stats(t))
    finally:
        plan.close()

    stamps, inners = [], []
    reg = fr.DeformableKinematicFilterReg(case.source, weights, args.sigma2)

    def cb(model):
        stamps.append(time.perf_counter())
        inners.append(model.inner_iterations)

    reg.set_callbacks([cb])
    res = reg.registration(case.target, maxiter=args.repeats + 2, tol=-1)
    d = np.diff(stamps)
    emit("  EM iteration of the device loop    %s   inner iterations %s" % (stats(d), inners[1:]))
    end = kc.rms(res.transformation.transform(case.source), case.moved)
    emit("  rms to the truth %.4g -> %.4g after %d iterations" % (kc.rms(case.source, case.moved), end, len(stamps)))


def restatement(case, args, emit):
    from oracle import filterreg_numpy as fo

    t0 = time.perf_counter()
    ok.skin(case.truth, case.pairs, case.vals, case.source)
    emit("  skin                               %10.3f ms" % ((time.perf_counter() - t0) * 1e3))
    ident = np.tile(np.eye(1, 8)[0], (case.n_nodes, 1))
    t0 = time.perf_counter()
    es = fo.expectation_step(case.source, case.target, case.target, args.sigma2, False)
    t1 = time.perf_counter()
    res = ok.maximization_step(case.source, case.target.shape[0], es.m0, es.m1, None, ident, case.pairs, case.vals,
                               args.sigma2)
    t2 = time.perf_counter()
    emit("  lattice E-step (oracle)            %10.3f ms" % ((t1 - t0) * 1e3))
    emit("  M-step, %2d inner iterations        %10.3f ms" % (res.n_iter, (t2 - t1) * 1e3))
    emit("  one EM iteration                   %10.3f ms" % ((t2 - t0) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=100000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--sigma2", type=float, default=1e-3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    case = kc.bar(args.m, args.k, 3, motion=4.0 / args.k)
    if args.restatement:
        emit("NumPy restatement (tests/oracle_kinematic.py) on the CPU, clustered bar M = N = %d, K = %d, sigma2 %g" % (args.m, args.k, args.sigma2))
        restatement(case, args, emit)
    else:
        emit("Deformable kinematic FilterReg on one GPU, clustered bar M = N = %d, K = %d, sigma2 %g, %d repeats" % (args.m, args.k, args.sigma2, args.repeats))
        gpu(case, args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
