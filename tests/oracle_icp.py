"""NumPy restatement of ICP as DESIGN.md section 3.15 defines it (moved points, the match with its tie rule, the ordered sums,
the point-to-point and point-to-plane steps, Open3D's loop), written from that definition and not from csrc/icp.hip.

The search is brute force in blocks of source rows.  Every decision value is one IEEE operation per step in the order the
definition writes it; the sums run over the matched source points in ascending order inside runs of RUN, the run sums are
added in ascending run order.  It also reports the decision gaps that say when a second implementation in plain IEEE
arithmetic must take the same discrete decisions, and the disagreement of two independent host solves of every step: the
yardstick of a third one.
"""
import numpy as np

from oracle_global_reg import REFIT_RUN as RUN, solve_bound

PIVOT = 1.0e-12          # a Cholesky pivot <= PIVOT max diag(A) is degenerate
POINT_TO_POINT, POINT_TO_PLANE = 0, 1
OK, TOO_FEW, DEGENERATE = 0, 1, 2
GAP = 1.0e-9
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def pose12(rot, t):
    return np.concatenate([np.asarray(rot, dtype=np.float64).reshape(9), np.asarray(t, dtype=np.float64).reshape(3)])


def moved(p, pose):
    """q_a = ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) + t_a."""
    q = np.empty_like(p)
    for a in range(3):
        q[:, a] = ((pose[3 * a] * p[:, 0] + pose[3 * a + 1] * p[:, 1]) + pose[3 * a + 2] * p[:, 2]) + pose[9 + a]
    return q


# -------------------------------------------------------------------------------------------------------------- search
def search(q, y, r, rows_per_block=256, gaps=False):
    """(index (M,) int32 with -1, d2 (M,) with +inf): the target of the smallest (d2, n) among d2 <= r r.  With ``gaps``
    also (least relative gap between best and second-best d2, least relative gap between a best d2 and r r)."""
    m = q.shape[0]
    idx = np.empty(m, dtype=np.int32)
    best = np.empty(m)
    r2 = r * r
    gap_second, gap_r = np.inf, np.inf
    for m0 in range(0, m, rows_per_block):
        blk = q[m0:m0 + rows_per_block]
        dx = y[None, :, 0] - blk[:, 0, None]
        dy = y[None, :, 1] - blk[:, 1, None]
        dz = y[None, :, 2] - blk[:, 2, None]
        d2 = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d2, axis=1)  # first minimum: the smaller index
        b = d2[np.arange(blk.shape[0]), j]
        idx[m0:m0 + blk.shape[0]] = j
        best[m0:m0 + blk.shape[0]] = b
        if gaps:
            if y.shape[0] > 1:
                two = np.partition(d2, 1, axis=1)[:, :2]
                with np.errstate(divide="ignore", invalid="ignore"):
                    g = (two[:, 1] - two[:, 0]) / two[:, 1]
                gap_second = min(gap_second, float(np.min(np.where(np.isnan(g), 0.0, g))))
            if np.isfinite(r2):
                gap_r = min(gap_r, float(np.min(np.abs(b - r2) / r2)))
    hit = best <= r2
    idx = np.where(hit, idx, -1).astype(np.int32)
    best = np.where(hit, best, np.inf)
    return (idx, best, gap_second, gap_r) if gaps else (idx, best)


# ---------------------------------------------------------------------------------------------------------------- sums
def ordered_sum(cols, matched):
    """Column sums of cols (M, k) over the matched rows: ascending m inside runs of RUN, run sums added in ascending order."""
    m, k = cols.shape
    nruns = -(-m // RUN)
    v = np.zeros((nruns * RUN, k))
    v[:m] = np.where(matched[:, None], cols, 0.0)  # + 0.0 is exact
    v = v.reshape(nruns, RUN, k)
    part = np.zeros((nruns, k))
    for u in range(RUN):
        part = part + v[:, u, :]
    total = np.zeros(k)
    for r in range(nruns):
        total = total + part[r]
    return total


def sums(kind, q, y, normals, idx, d2):
    """The raw sums of a step, 32 doubles laid out as prg_icp_sums writes them."""
    matched = idx >= 0
    j = np.where(matched, idx, 0)
    ym = y[j]
    one = np.ones(q.shape[0])
    dd = np.where(matched, d2, 0.0)
    out = np.zeros(32)
    if kind == POINT_TO_POINT:
        a = ordered_sum(np.column_stack([one, dd, q, ym]), matched)
        out[:8] = a
        if a[0] > 0.0:
            qc, yc = a[2:5] / a[0], a[5:8] / a[0]
        else:
            qc, yc = np.zeros(3), np.zeros(3)
        prod = [(q[:, i] - qc[i]) * (ym[:, k] - yc[k]) for i in range(3) for k in range(3)]
        out[8:17] = ordered_sum(np.column_stack(prod), matched)
        return out
    n = normals[j]
    res = (n[:, 0] * (q[:, 0] - ym[:, 0]) + n[:, 1] * (q[:, 1] - ym[:, 1])) + n[:, 2] * (q[:, 2] - ym[:, 2])
    jac = [q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0],
           n[:, 0], n[:, 1], n[:, 2]]
    cols = [one, dd] + [jac[i] * jac[k] for i in range(6) for k in range(i, 6)] + [jac[i] * res for i in range(6)]
    out[:29] = ordered_sum(np.column_stack(cols), matched)
    return out


# --------------------------------------------------------------------------------------------------------------- steps
def _delta_svd(hm, qc, yc):
    u, _, vt = np.linalg.svd(hm)
    dd = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, dd if dd != 0.0 else 1.0]) @ u.T
    return rot, yc - rot @ qc


def _delta_horn(s, qc, yc):
    n = np.array([[s[0, 0] + s[1, 1] + s[2, 2], s[1, 2] - s[2, 1], s[2, 0] - s[0, 2], s[0, 1] - s[1, 0]],
                  [s[1, 2] - s[2, 1], s[0, 0] - s[1, 1] - s[2, 2], s[0, 1] + s[1, 0], s[2, 0] + s[0, 2]],
                  [s[2, 0] - s[0, 2], s[0, 1] + s[1, 0], -s[0, 0] + s[1, 1] - s[2, 2], s[1, 2] + s[2, 1]],
                  [s[0, 1] - s[1, 0], s[2, 0] + s[0, 2], s[1, 2] + s[2, 1], -s[0, 0] - s[1, 1] + s[2, 2]]])
    _, vec = np.linalg.eigh(n)
    w, x, y, z = vec[:, 3]
    rot = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                    [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    return rot, yc - rot @ qc


def _unpack_plane(s):
    a = np.zeros((6, 6))
    k = 2
    for i in range(6):
        for j in range(i, 6):
            a[i, j] = a[j, i] = s[k]
            k += 1
    return a, -s[23:29]


def _cholesky(a, b):
    """x of a x = b, or None when a pivot is <= PIVOT max diag(a)."""
    low = np.zeros((6, 6))
    floor = PIVOT * np.max(np.diag(a))
    for k in range(6):
        d = a[k, k] - np.dot(low[k, :k], low[k, :k])
        if not d > floor:
            return None
        low[k, k] = np.sqrt(d)
        for i in range(k + 1, 6):
            low[i, k] = (a[i, k] - np.dot(low[i, :k], low[k, :k])) / low[k, k]
    w = np.zeros(6)
    for i in range(6):
        w[i] = (b[i] - np.dot(low[i, :i], w[:i])) / low[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = (w[i] - np.dot(low[i + 1:, i], x[i + 1:])) / low[i, i]
    return x


def _delta_from_x(x):
    """Open3D's TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0), shift x[3:]."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]])
    ry = np.array([[cb, 0.0, sb], [0.0, 1.0, 0.0], [-sb, 0.0, cb]])
    rz = np.array([[cg, -sg, 0.0], [sg, cg, 0.0], [0.0, 0.0, 1.0]])
    return rz @ ry @ rx, x[3:6].copy()


def _update(pose, rot, t):
    return pose12(rot @ pose[:9].reshape(3, 3), rot @ pose[9:] + t)


def step(kind, pose, s):
    """(new pose or None, status, disagreement): the step from the raw sums ``s`` and what a second, independent host solve of
    the same sums gives differently (largest difference of the 12 pose entries)."""
    cnt = s[0]
    if kind == POINT_TO_POINT:
        if cnt < 3.0:
            return None, TOO_FEW, 0.0
        qc, yc, hm = s[2:5] / cnt, s[5:8] / cnt, s[8:17].reshape(3, 3)
        new = _update(pose, *_delta_svd(hm, qc, yc))
        other = _update(pose, *_delta_horn(hm, qc, yc))
        return new, OK, float(np.max(np.abs(new - other)))
    if cnt < 6.0:
        return None, DEGENERATE, 0.0
    a, b = _unpack_plane(s)
    x = _cholesky(a, b)
    if x is None:
        return None, DEGENERATE, 0.0
    new = _update(pose, *_delta_from_x(x))
    other = _update(pose, *_delta_from_x(np.linalg.lstsq(a, b, rcond=None)[0]))
    return new, OK, float(np.max(np.abs(new - other)))


# ---------------------------------------------------------------------------------------------------------------- loop
def evaluate(src, tgt, pose, r, gaps=False):
    """dict of the matches at ``pose`` and their count K, ordered sum S, fitness and inlier_rmse."""
    q = moved(src, pose)
    found = search(q, tgt, r, gaps=gaps)
    idx, d2 = found[0], found[1]
    ks = ordered_sum(np.column_stack([np.ones(q.shape[0]), np.where(idx >= 0, d2, 0.0)]), idx >= 0)
    out = {"q": q, "index": idx, "d2": d2, "K": int(ks[0]), "S": float(ks[1]), "fitness": ks[0] / float(q.shape[0]),
           "inlier_rmse": float(np.sqrt(ks[1] / ks[0])) if ks[0] > 0.0 else 0.0}
    if gaps:
        out["gap_second"], out["gap_r"] = found[2], found[3]
    return out


def correspondences(idx):
    src = np.nonzero(idx >= 0)[0].astype(np.int32)
    return np.stack([src, idx[src]], axis=1).astype(np.int32)


def icp(src, tgt, r, kind=POINT_TO_POINT, normals=None, pose=None, max_iteration=30, relative_fitness=1.0e-6,
        relative_rmse=1.0e-6):
    """Open3D's loop.  dict: pose, n_iter (steps done), converged, status, the last evaluation (index, d2, K, S, fitness,
    inlier_rmse), correspondences, the least decision gaps along the trajectory and the largest disagreement of the two host
    solves of a step."""
    pose = IDENTITY.copy() if pose is None else np.array(pose, dtype=np.float64).reshape(12)
    ev = evaluate(src, tgt, pose, r, gaps=True)
    gap_second, gap_r = ev["gap_second"], ev["gap_r"]
    n_iter, converged, status, worst = 0, False, OK, 0.0
    for _ in range(max_iteration):
        new, status, dis = step(kind, pose, sums(kind, ev["q"], tgt, normals, ev["index"], ev["d2"]))
        if new is None:
            break
        worst = max(worst, dis)
        pose = new
        n_iter += 1
        nxt = evaluate(src, tgt, pose, r, gaps=True)
        gap_second, gap_r = min(gap_second, nxt["gap_second"]), min(gap_r, nxt["gap_r"])
        stop = abs(nxt["fitness"] - ev["fitness"]) < relative_fitness and abs(nxt["inlier_rmse"] - ev["inlier_rmse"]) < relative_rmse
        ev = nxt
        if stop:
            converged = True
            break
    out = dict(ev)
    out.update(pose=pose, rot=pose[:9].reshape(3, 3), t=pose[9:], n_iter=n_iter, converged=converged, status=status,
               correspondences=correspondences(ev["index"]), gap_second=gap_second, gap_r=gap_r, disagreement=worst)
    return out


def step_bound(disagreement):
    """What a third fp64 solve of a step may differ by (oracle_global_reg.solve_bound: 8 x the disagreement of the two host
    solves, floor 1e-12)."""
    return solve_bound(disagreement)


# --------------------------------------------------------------------------------------------------------------- cases
_CACHE = {}


def loop_case(name, synthetic):
    """The loop cases of the tests: (src, tgt, normals or None, kind, r, max_iteration, true (rot, t)) and, cached, the
    restatement's run.  ``synthetic``: the module that draws the clouds (handed in: this file does not import the product).
    Arrays are read-only."""
    if name not in _CACHE:
        if name == "pt2pl_plane" or name == "pt2pl_point":
            src, tgt, nrm, (rot, t) = synthetic.pt2pl_pair(1500, m=1200, seed=5)
            kind = POINT_TO_PLANE if name == "pt2pl_plane" else POINT_TO_POINT
            case = (src, tgt, nrm, kind, 0.1, 30, (rot, t))
        elif name == "filterreg_point":
            src, tgt, (rot, t) = synthetic.filterreg_pair(1500, m=1200, seed=7)
            case = (src, tgt, None, POINT_TO_POINT, 0.1, 50, (rot, t))
        elif name == "rigid_point":
            src, tgt, (rot, t, _) = synthetic.rigid_pair(1500, m=1200, seed=3)
            case = (src, tgt, None, POINT_TO_POINT, 0.5, 30, (rot, t))
        else:
            raise KeyError(name)
        for v in case[:3]:
            if v is not None:
                v.setflags(write=False)
        src, tgt, nrm, kind, r, max_it, _ = case
        _CACHE[name] = (case, icp(src, tgt, r, kind, nrm, max_iteration=max_it))
    return _CACHE[name]


LOOP_CASES = ("pt2pl_plane", "pt2pl_point", "filterreg_point", "rigid_point")
