"""NumPy restatement of global registration as DESIGN.md section 3.13 defines it (feature matching, hypothesis draws and
checks, scoring, refinement), written from that definition and not from csrc/global_reg.hip, plus the test families and the
band report that says when a second implementation in plain IEEE arithmetic must take the same discrete decisions.

Sums that the definition orders are accumulated in that order, one IEEE operation per step: D^2 over k ascending, scores over
c ascending inside segments of SCORE_SEGMENT correspondences with the segment sums added in ascending order.
"""
import functools

import numpy as np

SCORE_SEGMENT = 1024     # correspondences per segment of the scoring sum (a constant of the definition, not a launch parameter)
REFIT_RUN = 64           # correspondences per run of the refit's sums (ditto)
DEGENERATE = 0.05        # |e1 x e2| >= DEGENERATE |e1| |e2|
BAND = 1.0e-9

_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


# ------------------------------------------------------------------------------------------------------------ matching
def match(a, b, rows_per_block=512):
    """(index (na,) int32, d2 (na,)): the row of b of least D^2 for every row of a; ties go to the smaller index."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    na, d = a.shape
    idx = np.empty(na, dtype=np.int32)
    best = np.empty(na)
    for r0 in range(0, na, rows_per_block):
        blk = a[r0:r0 + rows_per_block]
        acc = np.zeros((blk.shape[0], b.shape[0]))
        for k in range(d):  # k ascending, every operation rounded once
            diff = blk[:, k][:, None] - b[:, k][None, :]
            acc = acc + diff * diff
        j = np.argmin(acc, axis=1)  # first minimum: the smaller index
        idx[r0:r0 + blk.shape[0]] = j
        best[r0:r0 + blk.shape[0]] = acc[np.arange(blk.shape[0]), j]
    return idx, best


def feature_matching(fa, fb, mutual=True):
    """(pairs (C, 2) int32 ascending in the source index, d2 (C,))."""
    iab, dab = match(fa, fb)
    keep = np.ones(iab.shape[0], dtype=bool)
    if mutual:
        iba, _ = match(fb, fa)
        keep = iba[iab] == np.arange(iab.shape[0])
    src = np.nonzero(keep)[0].astype(np.int32)
    return np.stack([src, iab[src]], axis=1).astype(np.int32), dab[src]


# --------------------------------------------------------------------------------------------------------------- draws
def draw(seed, h, c):
    """The triples (len(h), 3) int64 of the hypotheses ``h`` among ``c`` correspondences: splitmix64 on the counter 3h+j+1."""
    h = np.atleast_1d(np.asarray(h, dtype=np.uint64))
    out = np.empty((h.shape[0], 3), dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(3):
            ctr = np.uint64(3) * h + np.uint64(j + 1)
            z = np.uint64(seed) + _G * ctr
            z = (z ^ (z >> np.uint64(30))) * _M1
            z = (z ^ (z >> np.uint64(27))) * _M2
            z = z ^ (z >> np.uint64(31))
            out[:, j] = (((z >> np.uint64(32)) * np.uint64(c)) >> np.uint64(32)).astype(np.int64)
    return out


# -------------------------------------------------------------------------------------------------------------- Kabsch
def _norm3(v):
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])


def kabsch_svd(p, q):
    """Proper rotation and shift (no scale) that move p (n, 3) onto q (n, 3) in the least-squares sense; NumPy SVD."""
    pm, qm = p.sum(axis=0) / p.shape[0], q.sum(axis=0) / q.shape[0]
    hm = (p - pm).T @ (q - qm)
    u, _, vt = np.linalg.svd(hm)
    dd = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, dd if dd != 0.0 else 1.0]) @ u.T
    return rot, qm - rot @ pm


def kabsch_horn(p, q):
    """The same by Horn's unit-quaternion method: an independent host solve (eigenvector of a symmetric 4 x 4)."""
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    s = (p - pm).T @ (q - qm)
    n = np.array([[s[0, 0] + s[1, 1] + s[2, 2], s[1, 2] - s[2, 1], s[2, 0] - s[0, 2], s[0, 1] - s[1, 0]],
                  [s[1, 2] - s[2, 1], s[0, 0] - s[1, 1] - s[2, 2], s[0, 1] + s[1, 0], s[2, 0] + s[0, 2]],
                  [s[2, 0] - s[0, 2], s[0, 1] + s[1, 0], -s[0, 0] + s[1, 1] - s[2, 2], s[1, 2] + s[2, 1]],
                  [s[0, 1] - s[1, 0], s[2, 0] + s[0, 2], s[1, 2] + s[2, 1], -s[0, 0] - s[1, 1] + s[2, 2]]])
    _, vec = np.linalg.eigh(n)
    w, x, y, z = vec[:, 3]
    rot = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                    [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                    [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    return rot, qm - rot @ pm


# --------------------------------------------------------------------------------------------------------------- build
def build(p, q, seed, n_hyp, edge_similarity=0.9, h_offset=0, solver=kabsch_svd):
    """Hypotheses h_offset .. h_offset + n_hyp - 1: dict of triples (H, 3), valid (H,) bool, pose (H, 12) = (R row-major, t;
    zeros where invalid) and margin (H,): the least relative distance of a validity check of a distinct triple from its
    threshold (inf for a repeated index)."""
    c = p.shape[0]
    tri = draw(seed, np.arange(h_offset, h_offset + n_hyp, dtype=np.uint64), c)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    valid = distinct.copy()
    margin = np.full(n_hyp, np.inf)

    def check(lhs, rhs):
        nonlocal valid, margin
        valid &= lhs >= rhs
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.abs(lhs - rhs) / np.maximum(np.abs(lhs), np.abs(rhs))
        margin = np.where(distinct, np.minimum(margin, np.where(np.isnan(m), 0.0, m)), margin)

    for i, j in ((0, 1), (0, 2), (1, 2)):
        lp = _norm3(p[tri[:, j]] - p[tri[:, i]])
        lq = _norm3(q[tri[:, j]] - q[tri[:, i]])
        check(lp, edge_similarity * lq)
        check(lq, edge_similarity * lp)
    e1, e2 = p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]]
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    check(_norm3(cr), DEGENERATE * _norm3(e1) * _norm3(e2))
    pose = np.zeros((n_hyp, 12))
    for h in np.nonzero(valid)[0]:
        rot, t = solver(p[tri[h]], q[tri[h]])
        pose[h, :9], pose[h, 9:] = rot.reshape(9), t
    return {"triples": tri, "valid": valid, "pose": pose, "margin": margin}


# ------------------------------------------------------------------------------------------------------------- scoring
def residuals2(p, q, pose):
    """r^2 (H, C) of the poses (H, 12)."""
    pose = np.atleast_2d(pose)
    r = []
    for a in range(3):
        x = pose[:, 3 * a, None] * p[None, :, 0] + pose[:, 3 * a + 1, None] * p[None, :, 1] \
            + pose[:, 3 * a + 2, None] * p[None, :, 2] + pose[:, 9 + a, None] - q[None, :, a]
        r.append(x)
    return r[0] * r[0] + r[1] * r[1] + r[2] * r[2]


def ordered_sum(v):
    """Sum of the columns of v (H, C) as the definition orders it: ascending inside segments, segments ascending."""
    total = np.zeros(v.shape[0])
    for c0 in range(0, v.shape[1], SCORE_SEGMENT):
        s = np.zeros(v.shape[0])
        for c in range(c0, min(c0 + SCORE_SEGMENT, v.shape[1])):
            s = s + v[:, c]
        total = total + s
    return total


def score(p, q, pose, valid, tau):
    """(count (H,) int64 with -1 for an invalid hypothesis, sum (H,) with 0 there, band (int): r^2 of valid hypotheses within
    BAND tau^2 of tau^2)."""
    n_hyp = pose.shape[0]
    count = np.full(n_hyp, -1, dtype=np.int64)
    total = np.zeros(n_hyp)
    band = 0
    tau2 = tau * tau
    ids = np.nonzero(valid)[0]
    for b0 in range(0, ids.shape[0], 256):
        sel = ids[b0:b0 + 256]
        r2 = residuals2(p, q, pose[sel])
        inl = r2 <= tau2
        band += int(np.count_nonzero(np.abs(r2 - tau2) <= BAND * tau2))
        count[sel] = inl.sum(axis=1)
        total[sel] = ordered_sum(np.where(inl, r2, 0.0))  # + 0.0 is exact
    return count, total, band


def winner(count, total):
    """Index of the largest count, then the smallest sum, then the smallest h; -1 when no hypothesis is valid."""
    ok = np.nonzero(count >= 0)[0]
    if ok.shape[0] == 0:
        return -1
    order = np.lexsort((ok, total[ok], -count[ok]))
    return int(ok[order[0]])


# -------------------------------------------------------------------------------------------------------------- refine
def refine(p, q, pose, tau, iters):
    """(pose (12,), count, sum, inliers (indices), band, fitted): ``iters`` refits on the inliers of the current pose (a pose
    with fewer than 3 inliers is kept), then the inliers of the final pose; ``fitted``: the inliers the last refit ran on."""
    pose = np.array(pose, dtype=np.float64).reshape(12)
    tau2 = tau * tau
    band = 0
    fitted = np.zeros(0, dtype=np.int64)
    for _ in range(iters):
        r2 = residuals2(p, q, pose)[0]
        band += int(np.count_nonzero(np.abs(r2 - tau2) <= BAND * tau2))
        inl = np.nonzero(r2 <= tau2)[0]
        if inl.shape[0] < 3:
            break
        rot, t = kabsch_svd(p[inl], q[inl])
        pose = np.concatenate([rot.reshape(9), t])
        fitted = inl
    r2 = residuals2(p, q, pose)
    band += int(np.count_nonzero(np.abs(r2 - tau2) <= BAND * tau2))
    inl = r2[0] <= tau2
    return pose, int(inl.sum()), float(ordered_sum(np.where(inl, r2, 0.0)[0:1])[0]), np.nonzero(inl)[0], band, fitted


def ransac(p, q, tau, n_hyp, seed, edge_similarity=0.9, refine_iters=3):
    """All stages on correspondences (p, q): dict with the stage results, ``rot``, ``t``, ``fitness``, ``inlier_rmse``,
    ``inliers`` and ``band`` (the number of decisions inside the band, which must be 0 for an exact comparison)."""
    b = build(p, q, seed, n_hyp, edge_similarity)
    count, total, band = score(p, q, b["pose"], b["valid"], tau)
    w = winner(count, total)
    if w < 0:
        raise ValueError("no valid hypothesis")
    pose, cnt, sm, inl, band2, fitted = refine(p, q, b["pose"][w], tau, refine_iters)
    band += band2 + int(np.count_nonzero(b["margin"] <= BAND))
    return {"build": b, "count": count, "sum": total, "winner": w, "pose": pose, "rot": pose[:9].reshape(3, 3), "t": pose[9:],
            "fitness": cnt / float(p.shape[0]), "inlier_rmse": float(np.sqrt(sm / cnt)) if cnt else 0.0, "inliers": inl,
            "fitted": fitted, "final_count": cnt, "final_sum": sm, "band": band}


# ------------------------------------------------------------------------------------------------------------ families
def rotation_about(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


SHIFT = np.array([0.7, -1.3, 2.1])
ROT_S = rotation_about((1.0, 2.0, 3.0), 2.0)


@functools.lru_cache(maxsize=None)
def family_s(seed, sigma_f=0.33, n=1500):
    """Synthetic correspondences: dict of source / target points and descriptors (d = 33), the true pose, and the matched
    pairs with their points.  60 % of the source reappears in the target (moved, position noise 0.004, descriptor noise
    sigma_f), 40 % of the target is random; the target rows are shuffled."""
    rng = np.random.default_rng(1000 + seed)
    src = rng.uniform(-1.0, 1.0, (n, 3))
    fs = rng.uniform(0.0, 1.0, (n, 33))
    kept = rng.permutation(n)[:int(0.6 * n)]
    tgt = rng.uniform(-1.0, 1.0, (n, 3)) @ ROT_S.T + SHIFT
    ft = rng.uniform(0.0, 1.0, (n, 33))
    tgt[kept] = src[kept] @ ROT_S.T + SHIFT + rng.normal(0.0, 0.004, (kept.shape[0], 3))
    ft[kept] = fs[kept] + rng.normal(0.0, sigma_f, (kept.shape[0], 33))
    perm = rng.permutation(n)
    tgt, ft = np.ascontiguousarray(tgt[perm]), np.ascontiguousarray(ft[perm])
    pairs, d2 = feature_matching(fs, ft, True)
    out = {"source": src, "target": tgt, "source_feature": fs, "target_feature": ft, "rot": ROT_S, "t": SHIFT,
           "pairs": pairs, "d2": d2, "p": np.ascontiguousarray(src[pairs[:, 0]]), "q": np.ascontiguousarray(tgt[pairs[:, 1]])}
    for v in out.values():
        v.setflags(write=False)
    return out


S_HYP, S_TAU, S_SEED = 4096, 0.03, 7
F_HYP, F_TAU, F_SEED, F_RADII = 16384, 0.08, 0, (0.15, 0.3)
ROT_F_DEG = (140.0, 65.0)


def family_f_clouds(seed, n=2000):
    """Two independent samples of the C1 surface; the target turned by rot_zx(140, 65), shifted and with noise 0.003."""
    from probreg_amd import synthetic

    rot = synthetic.rot_zx(*ROT_F_DEG)
    src = synthetic.surface(n, seed)  # seed, seed + 1, seed + 2: as synthetic.rigid_pair draws its pair
    tgt = synthetic.surface(n, seed + 1) @ rot.T + SHIFT + np.random.default_rng(seed + 2).normal(0.0, 0.003, (n, 3))
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), rot, SHIFT


@functools.lru_cache(maxsize=None)
def family_s_ransac(seed):
    f = family_s(seed)
    return ransac(f["p"], f["q"], S_TAU, S_HYP, S_SEED)


def pose_error(rot, t, rot_true, t_true):
    """(rotation error in degrees, |t - t_true|)."""
    c = (np.trace(rot_true.T @ rot) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))), float(np.linalg.norm(t - t_true))


# ------------------------------------------------------------------------------------------------- stage cases of the GPU tests
BUILD_C, BUILD_H = (3, 64, 427), (1, 63, 4096)
SCORE_C, SCORE_H = (3, 65, 427), (1, 63, 4096)
CASE_SEED, CASE_TAU = 7, 0.03
TOL_FLOOR = 1.0e-12


@functools.lru_cache(maxsize=None)
def corr_case(c):
    """Correspondences (p, q) (c, 3): every pair a true one (moved by the pose of family S, noise 0.004) but, for c > 3,
    half of them with a random partner."""
    rng = np.random.default_rng(500 + c)
    p = rng.uniform(-1.0, 1.0, (c, 3))
    q = p @ ROT_S.T + SHIFT + rng.normal(0.0, 0.004, (c, 3))
    if c > 3:
        bad = rng.permutation(c)[:c // 2]
        q[bad] = rng.uniform(-1.0, 1.0, (bad.shape[0], 3)) @ ROT_S.T + SHIFT
    p.setflags(write=False)
    q.setflags(write=False)
    return p, q


@functools.lru_cache(maxsize=None)
def build_case(c, n_hyp):
    p, q = corr_case(c)
    return build(p, q, CASE_SEED, n_hyp)


def solver_disagreement(p, q, b):
    """Largest difference between the poses of two independent host solves (NumPy SVD, Horn's quaternions) over the valid
    hypotheses of a build: the yardstick of an fp64 solve of these triples.  0.0 when none is valid."""
    worst = 0.0
    for h in np.nonzero(b["valid"])[0]:
        rot, t = kabsch_horn(p[b["triples"][h]], q[b["triples"][h]])
        worst = max(worst, float(np.max(np.abs(np.concatenate([rot.reshape(9), t]) - b["pose"][h]))))
    return worst


def solve_bound(disagreement):
    """What a third fp64 solve may differ by: 8 x the disagreement of the two host solves, or TOL_FLOOR where that is larger
    (the rule of tests/test_tolerance_justification.py for fp64 solves)."""
    return max(8.0 * disagreement, TOL_FLOOR)


@functools.lru_cache(maxsize=None)
def score_case(c, n_hyp):
    """Explicit hypotheses for the scoring stage: the true pose of corr_case(c) turned by up to 0.03 rad about a random axis
    and shifted by N(0, 0.01), so that residuals lie on both sides of CASE_TAU; for n_hyp > 1 every fifth one is marked
    invalid.  Returns (pose (H, 12), valid (H,) bool, count, sum, band, winner)."""
    p, q = corr_case(c)
    rng = np.random.default_rng(900 + 7 * c + n_hyp)
    pose = np.empty((n_hyp, 12))
    for h in range(n_hyp):
        rot = rotation_about(rng.normal(size=3), rng.uniform(0.0, 0.03)) @ ROT_S
        pose[h, :9], pose[h, 9:] = rot.reshape(9), SHIFT + rng.normal(0.0, 0.01, 3)
    valid = np.ones(n_hyp, dtype=bool)
    if n_hyp > 1:
        valid[3::5] = False
    count, total, band = score(p, q, pose, valid, CASE_TAU)
    return pose, valid, count, total, band, winner(count, total)


def refit_condition(p, q, inliers):
    """Sensitivity of the rotation of a Kabsch solve to a perturbation of its cross-covariance: max(1, s1 / (s2 + s3)) of
    the singular values of the centred cross-covariance of the inliers."""
    pi, qi = p[inliers], q[inliers]
    s = np.linalg.svd((pi - pi.mean(axis=0)).T @ (qi - qi.mean(axis=0)), compute_uv=False)
    return max(1.0, float(s[0] / (s[1] + s[2])))


def refit_disagreement(p, q, inliers):
    """SVD against Horn on the final inlier set: the yardstick of the refit's solve."""
    r1, t1 = kabsch_svd(p[inliers], q[inliers])
    r2, t2 = kabsch_horn(p[inliers], q[inliers])
    return float(max(np.max(np.abs(r1 - r2)), np.max(np.abs(t1 - t2))))
