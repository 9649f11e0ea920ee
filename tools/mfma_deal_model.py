#!/usr/bin/env python
"""CPU model of how long a CULLING matrix-core column launch (csrc/cpd_sweeps_mfma.hip, k_colpass_mfma, grid mode) lasts at C1
when its S segments are contiguous runs of the streamed chunks and when chunk c is dealt to segment c mod S.
No GPU: numpy and scipy only.  These are predictions, not measurements.

    python tools/mfma_deal_model.py [--parent PAIRS_LOG] [--deal-only PAIRS_LOG] [--new PAIRS_LOG] > profiles/mfma_deal_model.txt

What goes in
  clouds     synthetic.rigid_pair(100000, seed=0), both in a kd order (median splits of the widest axis down to leaves of 32 points -
             the library's order differs in its tie breaks, not in kind), the source moved by the true transformation: the converged
             alignment, in which the window's later iterations run
  sigma2     of EM iterations 6 .. 16 as profiles/r6_c1_pairs_per_iteration.log has them
  the tests  the kernel's two box tests with its 2^-48 bound: a workgroup (512 targets) skips a chunk (256 sources) whose box is farther
             than (sqrt(largest column minimum of the workgroup) + motion)^2 + 48 / |kk|, a wave (128 targets) skips a group of 32 sources
             (two 16-point tiles) by the same rule with its own minimum; |kk| = log2(e) / (2 sigma2), motion = 0, column minimum =
             squared distance to the nearest source
  the chip   256 CUs x 3 workgroup slots, workgroups handed out in grid order (block index fastest) as slots come free, the workgroups
             of a CU share it equally (processor sharing)
  last block 100 000 = 195 x 512 + 160: the last block ends in pads.  Until this model was written it had no box and evaluated all 391
             chunks - 19 workgroups of 21 full chunks each (130 us of a CU alone, up to three times that shared), the last of them
             handed out near the end of the grid.  The model prices both: "last block: all" and "last block culls"
  the cost   a workgroup-chunk costs 0.2 us of staging plus 0.38 us per tile (the all-pairs sweep: 196 x 391 chunks x 16 tiles in 1.9 ms);
             its four waves meet at a barrier per chunk, so the tile count is the mean of the busiest wave's count and the four waves'
             average; "balanced waves" charges the average alone - what evening the waves out within a workgroup could gain at most
"""
import argparse
import heapq
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIGMA2 = {6: 3.26816e-02, 7: 2.14946e-02, 8: 1.41376e-02, 9: 9.29593e-03, 10: 6.11518e-03, 11: 4.02868e-03, 12: 2.66024e-03,
          13: 1.76209e-03, 14: 1.17198e-03, 16: 5.27973e-04}
CULL_EXP, LOG2E = 48.0, 1.4426950408889634
WG, WAVE, CHUNK, GROUP = 512, 128, 256, 32
CUS, SLOTS = 256, 3
T_STAGE, T_TILE = 0.2e-3, 0.38e-3  # ms


def kd_order(pts, leaf=32):
    idx = np.arange(len(pts))
    out = []
    stack = [idx]
    while stack:
        cur = stack.pop()
        if len(cur) <= leaf:
            out.append(cur)
            continue
        p = pts[cur]
        ax = int(np.argmax(p.max(axis=0) - p.min(axis=0)))
        half = (len(cur) // 2 + leaf - 1) // leaf * leaf  # whole leaves on the left
        part = np.argpartition(p[:, ax], half - 1)
        stack.append(cur[part[half:]])
        stack.append(cur[part[:half]])
    return np.concatenate(out)


def boxes(pts, size):
    """(lo, hi) of consecutive runs of `size` points; the last run may be short."""
    n = (len(pts) + size - 1) // size
    pad = np.concatenate([pts, np.repeat(pts[-1:], n * size - len(pts), axis=0)]).reshape(n, size, 3)
    return pad.min(axis=1), pad.max(axis=1)


def gap2(lo_a, hi_a, lo_b, hi_b):
    """Squared distance between every box of a and every box of b."""
    d = np.maximum(0.0, np.maximum(lo_a[:, None, :] - hi_b[None, :, :], lo_b[None, :, :] - hi_a[:, None, :]))
    return (d * d).sum(axis=2)


def needed_tiles(tgt, z, cmin, sigma2, last_block_culls):
    """tiles[b, c, w]: 16-point tiles of chunk c that wave w of block b evaluates (0 when the workgroup skips the chunk).
    last_block_culls False: the cloud's last block, which ends in pads, evaluates every chunk (the kernel before this model was
    written); True: it tests chunks with the box of its real points, its waves that hold pads test no groups."""
    reach = CULL_EXP * 2.0 * sigma2 / LOG2E
    nb, nc = (len(tgt) + WG - 1) // WG, (len(z) + CHUNK - 1) // CHUNK
    wlo, whi = boxes(tgt, WAVE)
    glo, ghi = boxes(z, GROUP)
    blo, bhi = boxes(tgt, WG)
    clo, chi = boxes(z, CHUNK)
    cm_w = np.array([cmin[i:i + WAVE].max() for i in range(0, len(tgt), WAVE)])
    cm_b = np.array([cmin[i:i + WG].max() for i in range(0, len(tgt), WG)])
    chunk_on = gap2(blo, bhi, clo, chi) <= (cm_b * 1.00001 + reach)[:, None]                    # [nb, nc]
    group_on = gap2(wlo, whi, glo, ghi) <= (cm_w * 1.00001 + reach)[:, None]                    # [waves, groups]
    ng = nc * (CHUNK // GROUP)
    g = np.zeros((nb * 4, ng), dtype=bool)
    g[:group_on.shape[0], :group_on.shape[1]] = group_on
    per_chunk = g.reshape(nb, 4, nc, CHUNK // GROUP).sum(axis=3) * 2                              # tiles per (block, wave, chunk)
    tiles = per_chunk.transpose(0, 2, 1) * chunk_on[:, :, None]
    if len(tgt) % WG:
        full_waves = (len(tgt) % WG) // WAVE
        tiles[-1, :, full_waves:] = 16 * chunk_on[-1][:, None]
        if not last_block_culls:
            tiles[-1] = 16
    return tiles


def makespan(costs):
    """costs[k]: workgroups in grid order.  256 CUs x 3 slots, processor sharing within a CU."""
    nxt = min(len(costs), CUS * SLOTS)
    cu_rem = [[] for _ in range(CUS)]
    for k in range(nxt):
        cu_rem[k % CUS].append(costs[k])
    cu_t = [0.0] * CUS
    heap = []
    for c in range(CUS):
        if cu_rem[c]:
            heapq.heappush(heap, (min(cu_rem[c]) * len(cu_rem[c]), c))
    end = 0.0
    while heap:
        t, c = heapq.heappop(heap)
        k = len(cu_rem[c])
        done = (t - cu_t[c]) / k
        rem = [r - done for r in cu_rem[c]]
        rem.remove(min(rem))
        cu_t[c] = t
        end = max(end, t)
        if nxt < len(costs):
            rem.append(costs[nxt])
            nxt += 1
        cu_rem[c] = rem
        if rem:
            heapq.heappush(heap, (t + max(min(rem), 0.0) * len(rem), c))
    return end


def launch_ms(tiles, segs, interleaved, balanced):
    nb, nc, _ = tiles.shape
    cps = (nc + segs - 1) // segs
    segs = (nc + cps - 1) // cps
    eff = tiles.mean(axis=2) if balanced else 0.5 * (tiles.max(axis=2) + tiles.mean(axis=2))
    cost = np.where(tiles.max(axis=2) > 0, T_STAGE + T_TILE * eff, 0.0)                         # [nb, nc]
    wg = np.zeros((segs, nb))
    for s in range(segs):
        sel = np.arange(s, nc, segs) if interleaved else np.arange(s * cps, min((s + 1) * cps, nc))
        wg[s] = cost[:, sel].sum(axis=1)
    return makespan(list(wg.reshape(-1)))  # (grid order: block index fastest)


def read_pairs_log(path):
    out = {}
    for line in open(path):
        p = line.split()
        if p and p[0].isdigit():
            out[int(p[0])] = (int(p[2]), float(p[6]), float(p[8]))  # matrix cores?, pairs, ms of the sweep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--segments", type=int, default=19)
    ap.add_argument("--parent", default="", help="bench.py --full --pairs-log table: contiguous deal, last block evaluates everything (measured column)")
    ap.add_argument("--deal-only", default="", help="... interleaved deal, last block evaluates everything")
    ap.add_argument("--new", default="", help="... interleaved deal, last block culls")
    args = ap.parse_args()
    from probreg_amd import synthetic

    src, tgt, (r, t, _s) = synthetic.rigid_pair(args.n, seed=0)
    z = src @ r.T + t
    z = z[kd_order(z)]
    tgt = tgt[kd_order(tgt)]
    cmin = cKDTree(z).query(tgt)[0] ** 2
    meas_p = read_pairs_log(args.parent) if args.parent else {}
    meas_d = read_pairs_log(args.deal_only) if args.deal_only else {}
    meas_n = read_pairs_log(args.new) if args.new else {}
    print("# tools/mfma_deal_model.py: C1 (N = M = %d), S = %d segments, 0.2 us + 0.38 us per tile, 256 CUs x 3 slots.  MODEL columns are" % (args.n, args.segments))
    print("# predictions of a CPU model; MEASURED columns are the sweep's ms of bench.py --full --pairs-log (`-`: that sweep did not run on the matrix cores)")
    print("#                                   | MODEL ms                                                                  | MEASURED ms")
    print("#                                   | last block: all           | last block culls                              |             interleaved  interleaved")
    print("# it  sigma2       pairs    pairs    | contiguous  interleaved   | contiguous  interleaved  +balanced waves       | contiguous  last: all    last: culls")
    print("#                  (model)  (meas.)  |")
    fmt = lambda m: ("%.4f" % m[2]).rjust(10) if m and m[0] == 1 else "-".rjust(10)
    for it in sorted(SIGMA2):
        old = needed_tiles(tgt, z, cmin, SIGMA2[it], False)
        new = needed_tiles(tgt, z, cmin, SIGMA2[it], True)
        ms = [launch_ms(t, args.segments, il, bal) for t, il, bal in ((old, False, False), (old, True, False), (new, False, False),
                                                                       (new, True, False), (new, True, True))]
        mp = meas_p.get(it)
        print("%4d  %.5e  %.3e %s | %8.3f    %8.3f      | %8.3f    %8.3f     %8.3f              | %s   %s   %s"
              % (it, SIGMA2[it], float(old.sum()) * WAVE * 16, ("%.3e" % mp[1]) if mp else "-".rjust(9), ms[0], ms[1], ms[2], ms[3], ms[4],
                 fmt(mp), fmt(meas_d.get(it)), fmt(meas_n.get(it))))

if __name__ == "__main__":
    main()
