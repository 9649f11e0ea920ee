#!/usr/bin/env python
"""A fixed, seeded walk through the branches of the CPD E-step driver (csrc/cpd_estep.hip), and the comparison of two kernel
traces of it: does a change to the driver launch the same kernels, in the same order, with the same grids?

    rocprofv3 --kernel-trace -d OUT -o t -- python tools/estep_launch_sequence.py        # the walk (tools/compare_launch_sequence.sh)
    python tools/estep_launch_sequence.py --compare OLD/t_results.db NEW/t_results.db    # exit status 0: identical

The engine decision is taken from counts of evaluated pairs, not from timings, so the sequence is deterministic.  Compared are the
ordered lists of (kernel name, grid, workgroup, LDS bytes) of every hardware queue.
"""
import os
import sqlite3
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def plan_for(src, tgt, cull=True):
    from probreg_amd.engine import CpdPlan

    plan = CpdPlan()
    plan.set_options(sort_source=True, sort_target=True, cull=cull)
    plan.set_source(src - src.mean(axis=0))
    plan.set_target(tgt - tgt.mean(axis=0))
    plan.init_sums()
    plan.init_params(None)
    return plan


def walk():
    import numpy as np

    from probreg_amd import _lib, bcpd, cpd, synthetic

    rigid = _lib.PRG_TF_RIGID
    big = synthetic.rigid_pair(40000, m=36000, seed=5)[:2]    # both clouds above the work queue's 32768 points
    mid = synthetic.rigid_pair(12000, m=11000, seed=6)[:2]    # above the matrix cores' 8192, below the queue's
    small = synthetic.rigid_pair(3000, m=2500, seed=7)[:2]

    def run(name, clouds, n_iter, setup=lambda plan: None, cull=True):
        plan = plan_for(clouds[0], clouds[1], cull)
        setup(plan)
        plan.iterate(rigid, True, 0.0, n_iter)
        print("%-28s sigma2 %.9e  fused %d  engines %s" % (name, plan.get_params()[13], plan.last_estep_fused(), plan.last_estep_engines()))
        plan.close()

    run("iterate", big, 40)                                                       # fused sweep, then the owner sweep
    run("two sweeps", big, 40, lambda p: p.set_moments_only(2))                   # column + (lean) row pass, then the work queue
    run("sparse engine 0", mid, 30, lambda p: p.set_sparse_engine(0))             # residual form over the grid of culled waves
    run("sparse engine 2", mid, 30, lambda p: p.set_sparse_engine(2))             # ... over the work queue
    run("sparse engine 2, two sweeps", mid, 30, lambda p: (p.set_sparse_engine(2), p.set_moments_only(2)))
    run("dense engine 0", mid, 25, lambda p: p.set_dense_engine(0))
    run("dense engine 2", mid, 25, lambda p: p.set_dense_engine(2))
    run("no cull, packed", small, 4, lambda p: p.set_tuning(2, 0, 4, 0), cull=False)
    run("no cull, scalar", small, 4, lambda p: p.set_tuning(-2, 0, -4, 0), cull=False)
    run("2-D", (mid[0][:, :2].copy(), mid[1][:, :2].copy()), 25)
    src, tgt = small
    res = bcpd.registration_bcpd(src[:1500], tgt[:1800], w=0.1, maxiter=6, tol=-1.0)              # per-source weights
    print("%-28s |v| max %.9e" % ("bcpd", float(np.max(np.abs(res.v)))))
    nsrc, ntgt = synthetic.nonrigid_pair(1800, m=1500, seed=8)
    res = cpd.registration_cpd(nsrc, ntgt, "nonrigid", maxiter=6, tol=-1.0)
    print("%-28s sigma2 %.9e" % ("non-rigid", res.sigma2))
    assert np.isfinite(res.sigma2)


def launches(path):
    cur = sqlite3.connect(path).cursor()
    cur.execute("select * from kernels order by start")
    cols = [d[0] for d in cur.description]
    want = [c for c in cols if c == "name" or c.startswith(("grid_", "workgroup_")) or "lds" in c.lower()]
    assert "name" in want and any("lds" in c.lower() for c in want) and len(want) >= 8, cols
    queue = cols.index("queue_id") if "queue_id" in cols else None
    per_queue = {}  # (dict order = first appearance)
    for row in cur.fetchall():
        per_queue.setdefault(row[queue] if queue is not None else 0, []).append(tuple(row[cols.index(c)] for c in want))
    return want, list(per_queue.values())


def compare(old, new):
    cols, a = launches(old)
    _, b = launches(new)
    print("compared per launch: %s" % ", ".join(cols))
    print("launches per queue: old %s, new %s" % ([len(q) for q in a], [len(q) for q in b]))
    if len(a) != len(b):
        print("DIFFERENT number of queues")
        return 1
    for k, (qa, qb) in enumerate(zip(a, b)):
        for i, (x, y) in enumerate(zip(qa, qb)):
            if x != y:
                print("queue %d, launch %d DIFFERS:\n  old %s\n  new %s" % (k, i, x, y))
                return 1
        if len(qa) != len(qb):
            print("queue %d: %d launches against %d" % (k, len(qa), len(qb)))
            return 1
    print("IDENTICAL launch sequences")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    walk()
