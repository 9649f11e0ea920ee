"""Vectorised NumPy restatement of DESIGN.md section 3.10: dual-quaternion skinning and the deformable kinematic
M-step of FilterReg (reference probreg/filterreg.py:38-42, 199-266; transformation.py:163-212), in both forms:

  complete (default)   diagonal blocks w_a^2 J^T J, cross blocks w_a w_b J^T J, gradient w_a J^T rx into BOTH nodes of a
                       point, points with m0 == 0 left out
  reference_form=True  exactly the reference: only the off-diagonal blocks (:228-236), the gradient into the first
                       node of a pair (:247-254), m0 == 0 -> float32 eps (:223)

TEST INFRASTRUCTURE: fp64 NumPy, no GPU, nothing imported from the product.
"""
from collections import namedtuple

import numpy as np

F32_EPS = float(np.finfo(np.float32).eps)
KinResult = namedtuple("KinResult", ["dualquats", "sigma2", "q", "n_iter", "twists"])


# ---- quaternions / dual quaternions, (..., 4) and (..., 8) arrays ----------------------------------------------------
def qmul(a, b):
    aw, ax, ay, az = np.moveaxis(np.asarray(a, dtype=np.float64), -1, 0)
    bw, bx, by, bz = np.moveaxis(np.asarray(b, dtype=np.float64), -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def qconj(a):
    return np.asarray(a, dtype=np.float64) * np.array([1.0, -1.0, -1.0, -1.0])


def rnorm(r):
    """|r| of rotation parts (..., 4)."""
    return np.sqrt(np.sum(np.square(r), axis=-1))


def dq_from_rt(r, t):
    """Rotation quaternion r (w, x, y, z) and translation t: d = (0, t) r / 2."""
    r = np.asarray(r, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    t4 = np.concatenate([np.zeros(t.shape[:-1] + (1,)), t], axis=-1)
    return np.concatenate([r, 0.5 * qmul(t4, r)], axis=-1)


def dq_from_axis_angle(axis, angle, t):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    return dq_from_rt(np.r_[np.cos(0.5 * angle), np.sin(0.5 * angle) * axis], t)


def dq_mul(a, b):
    """a * b applies b first."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.concatenate([qmul(a[..., :4], b[..., :4]), qmul(a[..., :4], b[..., 4:]) + qmul(a[..., 4:], b[..., :4])], axis=-1)


def dq_from_twist(tw):
    """filterreg.py:38-42 for one twist (6,) or many (K, 6)."""
    tw = np.asarray(tw, dtype=np.float64)
    if tw.ndim == 1:
        return dq_from_twist(tw[None])[0]
    ang = np.linalg.norm(tw[:, :3], axis=1)
    small = ang < F32_EPS
    safe = np.where(small, 1.0, ang)
    r = np.concatenate([np.cos(0.5 * safe)[:, None], np.sin(0.5 * safe)[:, None] * (tw[:, :3] / safe[:, None])], axis=1)
    r[small] = [1.0, 0.0, 0.0, 0.0]
    return dq_from_rt(r, tw[:, 3:])


def dq_transform(q, p):
    """Point transform of unit dual quaternions: vec(r (0, p) r*) + 2 vec(d r*)."""
    r, d = q[..., :4], q[..., 4:]
    p4 = np.concatenate([np.zeros(p.shape[:-1] + (1,)), p], axis=-1)
    return qmul(qmul(r, p4), qconj(r))[..., 1:] + 2.0 * qmul(d, qconj(r))[..., 1:]


def blend(dualquats, pairs, vals):
    """DLB: w0 q[pair0] + w1 q[pair1], both parts divided by |r| (no antipodal sign correction)."""
    dualquats = np.asarray(dualquats, dtype=np.float64).reshape(-1, 8)
    vals = np.asarray(vals, dtype=np.float64)
    b = vals[:, :1] * dualquats[pairs[:, 0]] + vals[:, 1:] * dualquats[pairs[:, 1]]
    return b / rnorm(b[:, :4])[:, None]


def skin(dualquats, pairs, vals, points):
    return dq_transform(blend(dualquats, pairs, vals), np.asarray(points, dtype=np.float64))


def jacobians(x):
    """se3_op.diff_x_from_twist (se3_op.py:56-59) per point: [-[x]x | I], (M, 3, 6)."""
    m = x.shape[0]
    j = np.zeros((m, 3, 6))
    j[:, 0, 1], j[:, 0, 2] = x[:, 2], -x[:, 1]
    j[:, 1, 0], j[:, 1, 2] = -x[:, 2], x[:, 0]
    j[:, 2, 0], j[:, 2, 1] = x[:, 1], -x[:, 0]
    j[:, :, 3:] = np.identity(3)
    return j


def _point_terms(t_source, n_target, m0, m1, sigma2, w, reference_form):
    """(live mask, s, mu, m0 as used, c)."""
    m = t_source.shape[0]
    c = w / (1.0 - w) * n_target / m  # :222 (sic: no (2 pi sigma2)^(3/2))
    m0 = np.array(m0, dtype=np.float64)
    m1 = np.asarray(m1, dtype=np.float64)
    live = np.ones(m, dtype=bool)
    if reference_form:
        m0[m0 == 0] = F32_EPS  # :223
    else:
        live = m0 != 0
    safe = np.where(live, m0, 1.0)
    m0m0 = np.where(live, safe / (safe + c), 0.0)
    s = np.sqrt(m0m0 * 1.0 / sigma2)
    mu = np.where(live[:, None], m1 / safe[:, None], 0.0)
    return live, s, mu, m0, c


def _scatter_blocks(a, rows, cols, blocks):
    """a[6r:6r+6, 6c:6c+6] += blocks, in point order."""
    for k in range(6):
        for l in range(6):
            np.add.at(a, (6 * rows + k, 6 * cols + l), blocks[:, k, l])


def normal_matrix(t_source, pairs, vals, s, n_nodes, reference_form):
    sj = s[:, None, None] * jacobians(t_source)
    jtj = np.einsum("mki,mkj->mij", sj, sj)
    a = np.zeros((6 * n_nodes, 6 * n_nodes))
    p0, p1 = pairs[:, 0], pairs[:, 1]
    w0, w1 = vals[:, 0].astype(np.float64), vals[:, 1].astype(np.float64)
    if reference_form:
        off = p0 != p1  # itertools.permutations: ordered pairs of DIFFERENT nodes only
        # (`w[0] * w[1]` of two f4 values is an f4 product in the reference, :233-234)
        w01 = (vals[:, 0].astype(np.float32) * vals[:, 1].astype(np.float32)).astype(np.float64)
        blk = w01[off, None, None] * jtj[off]
        _scatter_blocks(a, p0[off], p1[off], blk)
        _scatter_blocks(a, p1[off], p0[off], blk)  # (the same block, not its transpose: it is symmetric)
    else:
        for (ra, wa) in ((p0, w0), (p1, w1)):
            for (rb, wb) in ((p0, w0), (p1, w1)):
                _scatter_blocks(a, ra, rb, (wa * wb)[:, None, None] * jtj)
    return a


def gradient(t_source, pairs, vals, s, mu, twists, n_nodes, reference_form):
    """(b, rx) at the increments ``twists`` (K, 6)."""
    p0, p1 = pairs[:, 0], pairs[:, 1]
    w0, w1 = vals[:, 0].astype(np.float64), vals[:, 1].astype(np.float64)
    x = skin(dq_from_twist(twists), pairs, vals, t_source)
    if reference_form:
        x[p0 == p1] = 0.0  # never visited by the loop over permutations (:238-244)
    rx = s[:, None] * (x - mu)
    g = np.einsum("mki,mk->mi", s[:, None, None] * jacobians(t_source), rx)
    b = np.zeros(6 * n_nodes)
    if reference_form:
        off = p0 != p1
        for k in range(6):
            np.add.at(b, 6 * p0[off] + k, w0[off] * g[off, k])
    else:
        for k in range(6):
            np.add.at(b, 6 * p0 + k, w0 * g[:, k])
            np.add.at(b, 6 * p1 + k, w1 * g[:, k])
    return b, rx


def kinematic_system(t_source, n_target, m0, m1, pairs, vals, n_nodes, sigma2, w=0.0, reference_form=False):
    """(A, b at tw = 0)."""
    t_source = np.asarray(t_source, dtype=np.float64)
    pairs = np.asarray(pairs)
    _, s, mu, _, _ = _point_terms(t_source, n_target, m0, m1, sigma2, w, reference_form)
    a = normal_matrix(t_source, pairs, vals, s, n_nodes, reference_form)
    b, _ = gradient(t_source, pairs, vals, s, mu, np.zeros((n_nodes, 6)), n_nodes, reference_form)
    return a, b


def initial_q(t_source, n_target, m0, m1, pairs, vals, n_nodes, sigma2, w=0.0, reference_form=False):
    """q at zero increments: the scale of q."""
    t_source = np.asarray(t_source, dtype=np.float64)
    _, s, mu, _, _ = _point_terms(t_source, n_target, m0, m1, sigma2, w, reference_form)
    _, rx = gradient(t_source, np.asarray(pairs), np.asarray(vals), s, mu, np.zeros((n_nodes, 6)), n_nodes, reference_form)
    return float(np.dot(rx.T, rx).sum())


def maximization_step(t_source, n_target, m0, m1, m2, dualquats, pairs, vals, sigma2, w=0.0, maxiter=50, tol=1.0e-4,
                      reference_form=False, perturb=None):
    """One M-step of section 3.10.  ``perturb`` (a function of (A, b) -> (A, b)) is for conditioning measurements."""
    t_source = np.asarray(t_source, dtype=np.float64)
    pairs = np.asarray(pairs)
    vals = np.asarray(vals)
    dualquats = np.asarray(dualquats, dtype=np.float64).reshape(-1, 8)
    k = dualquats.shape[0]
    live, s, mu, m0u, c = _point_terms(t_source, n_target, m0, m1, sigma2, w, reference_form)
    if not live.any():
        return KinResult(dualquats, sigma2, None, 0, np.zeros((k, 6)))
    a = normal_matrix(t_source, pairs, vals, s, k, reference_form)
    tw = np.zeros(6 * k)
    n_iter = 0
    rx = None
    for _ in range(maxiter):
        b, rx = gradient(t_source, pairs, vals, s, mu, tw.reshape(k, 6), k, reference_form)
        aa, bb = (a, b) if perturb is None else perturb(a, b)
        dtw = np.linalg.lstsq(aa, bb, rcond=None)[0]
        tw -= dtw
        n_iter += 1
        if np.linalg.norm(dtw) < tol:
            break
    new = dq_mul(dq_from_twist(tw.reshape(k, 6)), dualquats)
    if m2 is not None:
        m1d, m2d = np.asarray(m1, dtype=np.float64), np.asarray(m2, dtype=np.float64)
        ts, a0, a1, a2 = t_source[live], m0u[live], m1d[live], m2d[live]  # (:263-264 over the points with m0 > 0)
        num = (a0 * np.square(ts).sum(axis=1) - 2.0 * (ts * a1).sum(axis=1) + a2) / (a0 + c)
        sigma2 = num.sum() / (3.0 * (a0 / (a0 + c)).sum())
    q = float(np.dot(rx.T, rx).sum())  # all nine entries (sic, :265)
    return KinResult(new, sigma2, q, n_iter, tw.reshape(k, 6))


def registration(source, target, pairs, vals, n_nodes, sigma2, update_sigma2=False, w=0.0, maxiter=50, tol=0.001,
                 min_sigma2=1.0e-4, reference_form=False, estep=None, history=None):
    """filterreg.py:120-147 with the kinematic model; ``estep(t_source, target, sigma2, update_sigma2)`` -> (m0, m1, m2)
    defaults to the oracle's lattice E-step.  Returns (dualquats, sigma2, q, iterations)."""
    if estep is None:
        from oracle import filterreg_numpy as fo

        def estep(ts, tgt, s2, upd):
            es = fo.expectation_step(ts, tgt, tgt, s2, upd)
            return es.m0, es.m1, es.m2

    source = np.asarray(source, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    dq = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]), (n_nodes, 1))
    q_prev, q, it = None, None, 0
    ret_sigma2 = sigma2
    for it in range(1, maxiter + 1):
        ts = skin(dq, pairs, vals, source)
        m0, m1, m2 = estep(ts, target, sigma2, update_sigma2)
        res = maximization_step(ts, target.shape[0], m0, m1, m2, dq, pairs, vals, sigma2, w, reference_form=reference_form)
        if res.q is None:
            q = q_prev
            break
        dq, ret_sigma2, q = res.dualquats, res.sigma2, res.q
        sigma2 = max(res.sigma2, min_sigma2)
        if history is not None:
            history.append((dq.copy(), sigma2, q, res.n_iter))
        if q_prev is not None and abs(q - q_prev) < tol:
            break
        q_prev = q
    return dq, ret_sigma2, q, it
