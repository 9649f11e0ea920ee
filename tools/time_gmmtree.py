#!/usr/bin/env python
"""Time GMMTree on one GPU: the tree build (per level: EM iterations, ms per iteration, total) and registration (ms per
iteration, total for maxiter iterations) on ``synthetic.surface`` clouds with a known 20 degree rotation.

    python tools/time_gmmtree.py [--sizes 10000,100000,1000000] [--levels 2,3,4] [--repeats 3] [--host-limit 60]

Each configuration is warmed up once, then timed ``--repeats`` times (median); every timed region ends in a device
synchronise (the build reads one q per EM iteration, the registration reads its moments every iteration).  The host
restatement (tests/oracle_gmmtree.py) is timed where one build + registration is predicted to take under
``--host-limit`` seconds (from a scaled first measurement at the smallest size).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from probreg_amd import gmmtree, synthetic  # noqa: E402


def clouds(n):
    src = synthetic.surface(n, 0)
    rot = synthetic.rot_zx(20.0, 0.0)
    tgt = synthetic.surface(n, 1) @ rot.T
    return src, tgt, rot


def time_gpu(src, tgt, level, maxiter):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = gmmtree.GMMTree(src, tree_level=level)
    torch.cuda.synchronize()
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = g.registration(tgt, maxiter=maxiter, tol=-1.0)
    torch.cuda.synchronize()
    t_reg = time.perf_counter() - t0
    iters = list(g.build_iterations)
    g.close()
    return t_build, t_reg, iters, res


def rot_err_deg(r_est, r_true):
    c = (np.trace(r_est.T @ r_true) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--levels", default="2,3,4")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=20)
    ap.add_argument("--host-limit", type=float, default=60.0)
    a = ap.parse_args()
    import oracle_gmmtree as og

    print("GMMTree timing on %s (fp64 tree path); synthetic.surface, target rotated 20 deg about z; registration "
          "maxiter=%d tol=-1" % (torch.cuda.get_device_name(0), a.maxiter))
    print("%8s %2s | %-22s %10s %10s | %10s %9s | %8s | %s" % ("N", "L", "build EM iters/level", "build ms", "ms/EM it",
                                                                 "reg ms", "ms/it", "rot err", "host build+reg s"))
    host_rate = None  # host seconds per (point x EM iteration x level-node) ~ crude predictor
    for n in [int(s) for s in a.sizes.split(",")]:
        src, tgt, rot = clouds(n)
        for lv in [int(s) for s in a.levels.split(",")]:
            time_gpu(src, tgt, lv, 2)  # warm-up (code objects, allocations, sort workspace)
            runs = [time_gpu(src, tgt, lv, a.maxiter) for _ in range(a.repeats)]
            tb = float(np.median([r[0] for r in runs]))
            tr = float(np.median([r[1] for r in runs]))
            iters = runs[0][2]
            err = rot_err_deg(runs[0][3].transformation.rot, rot)  # source -> target estimate vs the true rotation
            host = "-"
            work = n * sum(int(iters[l]) * 8 ** (l + 1) for l in range(lv))
            if host_rate is None or host_rate * work < a.host_limit:
                t0 = time.perf_counter()
                idx = og.init_indices(n, lv, 0)
                nodes, _ = og.build(src, lv, idx)
                plan = og.OracleGmmTreePlan()
                ref = gmmtree.GMMTree(tree_level=lv)
                ref._plan = plan
                ref.set_nodes(nodes)
                ref.registration(tgt, maxiter=a.maxiter, tol=-1.0)
                th = time.perf_counter() - t0
                host_rate = th / work
                host = "%.1f" % th
            print("%8d %2d | %-22s %10.1f %10.3f | %10.1f %9.3f | %8.3f | %s"
                  % (n, lv, ",".join(str(i) for i in iters), tb * 1e3, tb * 1e3 / sum(iters), tr * 1e3,
                     tr * 1e3 / a.maxiter, err, host), flush=True)


if __name__ == "__main__":
    main()
