"""NumPy restatement of DESIGN.md section 3.17: exact k-nearest-neighbour lists, radius counts and the two outlier filters,
written from that definition and not from csrc/icp.hip.

Brute force in blocks of query rows.  Every decision value is one IEEE operation per step in the order the definition writes
it: d2 = (dx dx + dy dy) + dz dz with dx = y_n,0 - q_0; lists by lexsort on (d2, n) among d2 <= r r; the mean neighbour distance
added in list order from 0.0; the two sums of the statistical filter in runs of RUN consecutive points, the run sums added in
ascending run order.  It also reports the decision gaps that say when a second implementation in plain IEEE arithmetic must
take the same discrete decisions.
"""
import numpy as np

from oracle_global_reg import REFIT_RUN as RUN

MAX_K = 64
GAP = 1.0e-9  # a decision nearer than this (relative) to its threshold may be excused; the cap on excused points is 0


def d2_block(q, y):
    """(rows of q, N): d2 = (dx dx + dy dy) + dz dz, dx = y_n,0 - q_0."""
    dx = y[None, :, 0] - q[:, 0, None]
    dy = y[None, :, 1] - q[:, 1, None]
    dz = y[None, :, 2] - q[:, 2, None]
    return (dx * dx + dy * dy) + dz * dz


def knn(q, y, k, r=np.inf, rows_per_block=256):
    """(index (Q, k) int32, d2 (Q, k), count (Q,) int32): per query the n with d2 <= r r in ascending (d2, n), cut to k;
    the slots past count hold -1 and +inf."""
    assert 1 <= k <= MAX_K and r > 0.0
    nq, n = q.shape[0], y.shape[0]
    r2 = r * r
    idx = np.full((nq, k), -1, dtype=np.int32)
    out = np.full((nq, k), np.inf)
    cnt = np.zeros(nq, dtype=np.int32)
    ids = np.arange(n)
    for m0 in range(0, nq, rows_per_block):
        d2 = d2_block(q[m0:m0 + rows_per_block], y)
        for i in range(d2.shape[0]):
            row = d2[i]
            order = np.lexsort((ids, row))  # by d2, then by n
            order = order[row[order] <= r2][:k]
            c = order.shape[0]
            idx[m0 + i, :c] = order
            out[m0 + i, :c] = row[order]
            cnt[m0 + i] = c
    return idx, out, cnt


def radius_count(q, y, r, rows_per_block=256, gap=False):
    """(Q,) int32: #{n : d2 <= r r}.  With ``gap`` also the least |d2 - r r| / (r r) over all pairs."""
    r2 = r * r
    cnt = np.empty(q.shape[0], dtype=np.int32)
    least = np.inf
    for m0 in range(0, q.shape[0], rows_per_block):
        d2 = d2_block(q[m0:m0 + rows_per_block], y)
        cnt[m0:m0 + d2.shape[0]] = np.sum(d2 <= r2, axis=1)
        if gap:
            least = min(least, float(np.min(np.abs(d2 - r2) / r2)))
    return (cnt, least) if gap else cnt


def run_sum(v):
    """Sum of v (n,): ascending inside runs of RUN from 0.0, then the run sums in ascending run order from 0.0."""
    n = v.shape[0]
    nruns = -(-n // RUN)
    w = np.zeros(nruns * RUN)
    w[:n] = v  # + 0.0 is exact
    w = w.reshape(nruns, RUN)
    part = np.zeros(nruns)
    for u in range(RUN):
        part = part + w[:, u]
    total = 0.0
    for r in range(nruns):
        total = total + part[r]
    return float(total)


def mean_distances(d2, cnt):
    """a_i = (sum of sqrt(d2) over the list, in list order from 0.0) / its length."""
    a = np.zeros(d2.shape[0])
    for t in range(d2.shape[1]):
        a = a + np.where(t < cnt, np.sqrt(np.where(t < cnt, d2[:, t], 0.0)), 0.0)  # + 0.0 is exact
    return a / cnt


def statistical(points, k, std_ratio):
    """dict: mask, index, score (a_i), mu, s, thr, and gap: the least |a_i - thr| / thr."""
    n = points.shape[0]
    _, d2, cnt = knn(points, points, k)
    assert np.all(cnt == min(k, n))
    a = mean_distances(d2, cnt)
    mu = run_sum(a) / n
    e = a - mu
    s = float(np.sqrt(run_sum(e * e) / (n - 1))) if n > 1 else 0.0
    scaled = std_ratio * s
    thr = mu + scaled
    mask = a <= thr
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = float(np.min(np.abs(a - thr) / thr)) if thr > 0.0 else 0.0
    return {"mask": mask, "index": np.nonzero(mask)[0].astype(np.int32), "score": a, "mu": mu, "s": s, "thr": thr, "gap": gap}


def radius(points, nb_points, r):
    """dict: mask, index, score (c_i, the point itself counted), and gap: the least |d2 - r r| / (r r) over all pairs."""
    c, gap = radius_count(points, points, r, gap=True)
    mask = c > nb_points
    return {"mask": mask, "index": np.nonzero(mask)[0].astype(np.int32), "score": c, "gap": gap}


# --------------------------------------------------------------------------------------------------------------- cases
_CACHE = {}


def cached(key, fn):
    """The value of fn() under ``key``, computed once; arrays in it are made read-only."""
    if key not in _CACHE:
        val = fn()
        for v in (val.values() if isinstance(val, dict) else val if isinstance(val, tuple) else (val,)):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def filter_cloud(synthetic):
    """The cloud of the filter tests: the target of filterreg_pair(2000, seed=0), which has 100 uniform outliers.
    ``synthetic``: the module that draws the clouds (handed in: this file does not import the product)."""
    return cached("filter_cloud", lambda: np.ascontiguousarray(synthetic.filterreg_pair(2000, seed=0)[1]))
