"""NumPy restatement of generalized ICP as DESIGN.md section 3.16 defines it (the covariance of a unit normal, the per-pair
matrix M = C_target + R C_source R^T and its inverse by the adjugate, the weighted 6 x 6 system, the Mahalanobis objective),
written from that definition and not from csrc/icp.hip.  The search, the ordered sums and the evaluation are those of section 3.15
and come from oracle_icp; the Cholesky step and the pose update are restated here in the order of the one lane that takes them.

Every value is one IEEE operation per step in the order the definition writes it.  Covariances are (n, 6): xx, xy, xz, yy, yz,
zz.  ``step`` solves every system a second time on the host (lstsq) and reports the disagreement: the yardstick of a third
solve.  ``inverse_disagreement`` does the same for the per-pair inverse (adjugate against a Cholesky inverse).
"""
import numpy as np

import oracle_icp as oi

GENERALIZED = 2
EPSILON = 1.0e-3


# --------------------------------------------------------------------------------------------------------- covariances
def covariances_from_normals(normals, epsilon=EPSILON):
    """(n, 6): C = I - (1 - epsilon) u u^T, u = n / |n| with |n| = sqrt((n0 n0 + n1 n1) + n2 n2); w = (1 - epsilon) u,
    C_aa = 1 - w_a u_a, C_ab = -(w_a u_b) for a < b."""
    n = np.asarray(normals, dtype=np.float64)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    u = np.stack([n[:, 0] / length, n[:, 1] / length, n[:, 2] / length], axis=1)
    k = 1.0 - epsilon
    w = np.stack([k * u[:, 0], k * u[:, 1], k * u[:, 2]], axis=1)
    c = np.empty((n.shape[0], 6))
    c[:, 0] = 1.0 - w[:, 0] * u[:, 0]
    c[:, 1] = -(w[:, 0] * u[:, 1])
    c[:, 2] = -(w[:, 0] * u[:, 2])
    c[:, 3] = 1.0 - w[:, 1] * u[:, 1]
    c[:, 4] = -(w[:, 1] * u[:, 2])
    c[:, 5] = 1.0 - w[:, 2] * u[:, 2]
    return c


_SYM = ((0, 1, 2), (1, 3, 4), (2, 4, 5))  # the slot of entry (a, b) of a symmetric matrix


def full(c6):
    """(n, 3, 3) of (n, 6)."""
    return c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


# ------------------------------------------------------------------------------------------------------------ per pair
def pair_matrix(pose, cs, ct):
    """M (n, 6) = C_target + (R C_source) R^T, upper triangle: (R C)_ab = (R_a0 C_0b + R_a1 C_1b) + R_a2 C_2b,
    (R C R^T)_ab = ((RC)_a0 R_b0 + (RC)_a1 R_b1) + (RC)_a2 R_b2, M_ab = C_target,ab + that."""
    rc = [[(pose[3 * a] * cs[:, _SYM[0][b]] + pose[3 * a + 1] * cs[:, _SYM[1][b]]) + pose[3 * a + 2] * cs[:, _SYM[2][b]]
           for b in range(3)] for a in range(3)]
    m = np.empty_like(ct)
    for a in range(3):
        for b in range(a, 3):
            s = _SYM[a][b]
            m[:, s] = ct[:, s] + ((rc[a][0] * pose[3 * b] + rc[a][1] * pose[3 * b + 1]) + rc[a][2] * pose[3 * b + 2])
    return m


def inverse(m):
    """P (n, 6) = adj(M) / det(M), one division per entry."""
    m00, m01, m02, m11, m12, m22 = (m[:, k] for k in range(6))
    c00 = m11 * m22 - m12 * m12
    c01 = m02 * m12 - m01 * m22
    c02 = m01 * m12 - m02 * m11
    c11 = m00 * m22 - m02 * m02
    c12 = m01 * m02 - m00 * m12
    c22 = m00 * m11 - m01 * m01
    det = (m00 * c00 + m01 * c01) + m02 * c02
    return np.stack([c00 / det, c01 / det, c02 / det, c11 / det, c12 / det, c22 / det], axis=1)


def inverse_disagreement(m):
    """Largest difference, relative to the largest entry of the inverse, between the adjugate inverse and a Cholesky inverse
    of the same matrices."""
    p = full(inverse(m))
    low = np.linalg.cholesky(full(m))
    li = np.linalg.inv(low)
    other = li.transpose(0, 2, 1) @ li
    return float(np.max(np.abs(p - other)) / np.max(np.abs(p)))


def _cross(q, p):
    """q x p, columns."""
    return [q[1] * p[2] - q[2] * p[1], q[2] * p[0] - q[0] * p[2], q[0] * p[1] - q[1] * p[0]]


def pair_terms(q, y, p6):
    """The 28 columns of a pair behind slots 2 .. 29: J = (-[q]x | I), d = q - y.  B = P (-[q]x) has the rows q x P_a;
    E = (-[q]x)^T B has the columns q x B_.b; v = P d; the rotation part of J^T P d is q x v."""
    qc = [q[:, 0], q[:, 1], q[:, 2]]
    d = [q[:, a] - y[:, a] for a in range(3)]
    p = [[p6[:, _SYM[a][b]] for b in range(3)] for a in range(3)]
    bm = [_cross(qc, p[a]) for a in range(3)]
    v = [(p[a][0] * d[0] + p[a][1] * d[1]) + p[a][2] * d[2] for a in range(3)]
    em = [[None] * 3 for _ in range(3)]
    for b in range(3):
        col = _cross(qc, [bm[0][b], bm[1][b], bm[2][b]])
        for a in range(3):
            em[a][b] = col[a]
    cols = []
    for a in range(3):  # rows 0 .. 2 of the upper triangle: E_ab (b >= a), then (J^T P J)_{a, 3 + b} = B_ba
        cols += [em[a][b] for b in range(a, 3)]
        cols += [bm[b][a] for b in range(3)]
    for a in range(3):  # rows 3 .. 5: P_ab (b >= a)
        cols += [p[a][b] for b in range(a, 3)]
    cols += _cross(qc, v) + v
    cols.append((d[0] * v[0] + d[1] * v[1]) + d[2] * v[2])
    return cols


# ---------------------------------------------------------------------------------------------------------------- sums
def sums(pose, q, y, cs, ct, idx, d2):
    """The raw sums of a generalized step, 32 doubles laid out as prg_icp_sums writes them: count, sum d2, the upper triangle of
    sum J^T P J (21), sum J^T P d (6), sum d^T P d."""
    matched = idx >= 0
    j = np.where(matched, idx, 0)
    p6 = inverse(pair_matrix(pose, cs, ct[j]))
    cols = [np.ones(q.shape[0]), np.where(matched, d2, 0.0)] + pair_terms(q, y[j], p6)
    out = np.zeros(32)
    out[:30] = oi.ordered_sum(np.column_stack(cols), matched)
    return out


def cholesky_in_order(a, b):
    """x of a x = b by Cholesky with every subtraction in ascending column order (section 3.15 names the factorisation, this
    is the order the one lane takes), or None when a pivot is <= PIVOT max diag(a).  oracle_icp._cholesky is the same
    factorisation with np.dot for the inner products; the two differ by roundings only."""
    low = np.zeros((6, 6))
    floor = oi.PIVOT * max(a[k, k] for k in range(6))
    for k in range(6):
        d = a[k, k]
        for j in range(k):
            d = d - low[k, j] * low[k, j]
        if not d > floor:
            return None
        low[k, k] = np.sqrt(d)
        for i in range(k + 1, 6):
            v = a[i, k]
            for j in range(k):
                v = v - low[i, j] * low[k, j]
            low[i, k] = v / low[k, k]
    w = np.zeros(6)
    for i in range(6):
        v = b[i]
        for j in range(i):
            v = v - low[i, j] * w[j]
        w[i] = v / low[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        v = w[i]
        for j in range(i + 1, 6):
            v = v - low[j, i] * x[j]
        x[i] = v / low[i, i]
    return x


def update_in_order(pose, x):
    """The pose after the step x: dR = Rz(x2) Ry(x1) Rx(x0) entry by entry, products left to right; R <- dR R and
    t <- dR t + dt with (a b + c d) + e f sums.  Differs from oracle_icp._update(pose, *_delta_from_x(x)) by roundings only -
    and equals the device bit for bit only where the two sines and cosines do."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    d = [cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
         sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
         -sb, cb * sa, cb * ca]
    new = np.empty(12)
    for a in range(3):
        for b in range(3):
            new[3 * a + b] = (d[3 * a] * pose[b] + d[3 * a + 1] * pose[3 + b]) + d[3 * a + 2] * pose[6 + b]
        new[9 + a] = ((d[3 * a] * pose[9] + d[3 * a + 1] * pose[10]) + d[3 * a + 2] * pose[11]) + x[3 + a]
    return new


def step(pose, s):
    """(new pose or None, status, disagreement) from the raw sums: slots 0 .. 28 are laid out as point-to-plane's.  The pose
    comes from the ordered solve; the disagreement is the largest difference of the 12 pose entries to two other host solves
    of the same sums (oracle_icp's Cholesky with np.dot, and lstsq)."""
    if s[0] < 6.0:
        return None, oi.DEGENERATE, 0.0
    a, b = oi._unpack_plane(s)
    x = cholesky_in_order(a, b)
    if x is None or oi._cholesky(a, b) is None:
        return None, oi.DEGENERATE, 0.0
    new = update_in_order(pose, x)
    others = [oi._update(pose, *oi._delta_from_x(oi._cholesky(a, b))),
              oi._update(pose, *oi._delta_from_x(np.linalg.lstsq(a, b, rcond=None)[0]))]
    return new, oi.OK, float(max(np.max(np.abs(new - o)) for o in others))


# ---------------------------------------------------------------------------------------------------------------- loop
def gicp(src, tgt, r, cs, ct, pose=None, max_iteration=30, relative_fitness=1.0e-6, relative_rmse=1.0e-6):
    """Open3D's loop with the generalized step; the evaluation and the stop test are Euclidean (oracle_icp.evaluate).  dict as
    oracle_icp.icp, plus ``objective`` (slot 29 at the last evaluation) and ``margin``: how far the last stop test was from
    flipping, min over the two criteria of | |change| - threshold |."""
    pose = oi.IDENTITY.copy() if pose is None else np.array(pose, dtype=np.float64).reshape(12)
    ev = oi.evaluate(src, tgt, pose, r, gaps=True)
    gap_second, gap_r = ev["gap_second"], ev["gap_r"]
    n_iter, converged, status, worst, margin = 0, False, oi.OK, 0.0, np.inf
    for _ in range(max_iteration):
        new, status, dis = step(pose, sums(pose, ev["q"], tgt, cs, ct, ev["index"], ev["d2"]))
        if new is None:
            break
        worst = max(worst, dis)
        pose = new
        n_iter += 1
        nxt = oi.evaluate(src, tgt, pose, r, gaps=True)
        gap_second, gap_r = min(gap_second, nxt["gap_second"]), min(gap_r, nxt["gap_r"])
        df, dr = abs(nxt["fitness"] - ev["fitness"]), abs(nxt["inlier_rmse"] - ev["inlier_rmse"])
        stop = df < relative_fitness and dr < relative_rmse
        margin = min(abs(df - relative_fitness), abs(dr - relative_rmse))
        ev = nxt
        if stop:
            converged = True
            break
    out = dict(ev)
    out.update(pose=pose, rot=pose[:9].reshape(3, 3), t=pose[9:], n_iter=n_iter, converged=converged, status=status,
               correspondences=oi.correspondences(ev["index"]), gap_second=gap_second, gap_r=gap_r, disagreement=worst,
               margin=margin, objective=float(sums(pose, ev["q"], tgt, cs, ct, ev["index"], ev["d2"])[29]))
    return out


# --------------------------------------------------------------------------------------------------------------- cases
_CACHE = {}
LOOP_CASES = ("gicp_r0.1", "gicp_r0.05")


def loop_clouds(synthetic):
    """pt2pl_pair(1500, m=1200, seed=5) with the source's analytic normals rounded through float32: (src, tgt, source normals,
    target normals, true (rot, t)).  Read-only."""
    if "clouds" not in _CACHE:
        src, tgt, tn, true = synthetic.pt2pl_pair(1500, m=1200, seed=5)
        sn = synthetic.surface_with_normals(1200, 5)[1].astype(np.float32).astype(np.float64)
        for v in (src, tgt, sn, tn):
            v.setflags(write=False)
        _CACHE["clouds"] = (src, tgt, sn, tn, true)
    return _CACHE["clouds"]


def loop_case(name, synthetic):
    """((src, tgt, source normals, target normals, r, max_iteration, true (rot, t)), the restatement's run), cached."""
    if name not in _CACHE:
        src, tgt, sn, tn, true = loop_clouds(synthetic)
        r = {"gicp_r0.1": 0.1, "gicp_r0.05": 0.05}[name]
        cs, ct = covariances_from_normals(sn), covariances_from_normals(tn)
        _CACHE[name] = ((src, tgt, sn, tn, r, 30, true), gicp(src, tgt, r, cs, ct, max_iteration=30))
    return _CACHE[name]
