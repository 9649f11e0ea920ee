#!/usr/bin/env python
"""Time CpdPlan.correspondences (csrc/cpd_correspond.hip) on one MI355X: the C1 clouds (synthetic.rigid_pair, seed 0)
at M = N = 10^4 and 10^5, ten rigid EM iterations into their registration, k = 1, 4 and 8, both sides - against the brute-force
nearest-neighbour sweep of prg_nn_mean_distance (mu.compute_rmse) on the same two clouds, which does the same loads and one `min` per
pair.  Writes profiles/correspond_timing.txt (or --out).

Every figure is a whole call on a host clock: the calls end in a device-to-host copy, i.e. they are synchronous.  That includes the
calls' own allocations and read-backs on both sides of the comparison; the yardstick is the C entry point itself on float32 arrays
prepared once (it uploads its two clouds per call, 2.4 MB at 10^5; the plan call uploads nothing).  A sample is the mean of several
back-to-back calls (20 at 10^4, 3 at 10^5); per size the variants are sampled in interleaved rounds in one process, and median and
minimum over the rounds are reported.  Kernel times proper come from a kernel trace of this script (rocprofv3 --kernel-trace --stats
... -- python tools/correspond_timing.py --sizes 100000 --rounds 1), taken in a run of its own.  The share of
peak is (pairs x vector instructions per pair / the fp32 vector issue rate) / time, with the MI355X's 157.3 TFLOP/s counted as
78.65e12 lane-instructions per second (an FMA is one instruction) and the instructions per pair the algorithm needs: 3 subtractions, a
multiplication, 2 FMAs for d^2, then an FMA, an addition and a compare for the score (9) - the yardstick: d^2 and a minimum (7)."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from probreg_amd import _lib, cpd, synthetic  # noqa: E402
from probreg_amd.engine import _current_device_and_stream  # noqa: E402

LANE_RATE = 157.3e12 / 2.0
INSTR_SWEEP, INSTR_NN = 9, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correspond_timing.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    lines = ["# tools/correspond_timing.py: whole synchronous calls (mean of 20 / 3 back-to-back calls per sample at 10^4 / 10^5), "
             "%d interleaved rounds after 2 warm-up rounds" % args.rounds,
             "# share of peak: pairs x instructions per pair / 78.65e12 lane-instructions/s, over the median time",
             "# %-8s %-28s %12s %12s %10s %12s" % ("M = N", "call", "median ms", "min ms", "of peak", "x yardstick")]
    for n in args.sizes:
        src, tgt, _ = synthetic.rigid_pair(n, seed=0)
        reg = cpd.RigidCPD(src)
        reg._initialize(tgt)
        plan = reg._plan
        plan.set_moments_only(2)
        for _ in range(10):
            plan.estep(0.0)
            plan.mstep(_lib.PRG_TF_RIGID, True)
        plan.estep(0.0)
        z = np.ascontiguousarray(plan.get_tsource(), dtype=np.float32)
        x = np.ascontiguousarray(tgt - reg._cx, dtype=np.float32)
        dev, st = _current_device_and_stream()
        out = ctypes.c_double(0.0)

        def yardstick():
            _lib.check(_lib.lib.prg_nn_mean_distance(dev, ctypes.c_void_p(st), _lib.ptr(z), n, _lib.ptr(x), n, 3, ctypes.byref(out)))

        inner = 20 if n <= 20000 else 3
        variants = [("nn_mean_distance (yardstick)", INSTR_NN, yardstick)]
        for side in ("source", "target"):
            for k in (1, 4, 8):
                variants.append(("correspondences k=%d %s" % (k, side), INSTR_SWEEP,
                                 lambda k=k, side=side: plan.correspondences(k, side)))
        times = [[] for _ in variants]
        for r in range(args.rounds + 2):
            for i, (_name, _instr, fn) in enumerate(variants):
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                dt = (time.perf_counter() - t0) / inner
                if r >= 2:
                    times[i].append(dt)
        pairs = float(n) * float(n)
        base = float(np.median(times[0]))
        for (name, instr, _fn), ts in zip(variants, times):
            med, mn = float(np.median(ts)), float(np.min(ts))
            lines.append("  %-8d %-28s %12.3f %12.3f %9.1f%% %12.2f" % (n, name, med * 1e3, mn * 1e3,
                                                                     100.0 * pairs * instr / LANE_RATE / med, med / base))
        lines.append("# rounds in ms, in the order they ran (one line per call, one column per round):")
        for (name, _instr, _fn), ts in zip(variants, times):
            lines.append("#   %-8d %-28s %s" % (n, name, " ".join("%.2f" % (t * 1e3) for t in ts)))
        plan.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
