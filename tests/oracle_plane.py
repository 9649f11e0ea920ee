"""NumPy restatement of plane segmentation as DESIGN.md section 3.20 defines it (draw, validity, the plane of a triple, the
anchored distance, scoring, the winner, the refits, ``segment_planes``), written from that definition and not from
csrc/plane_seg.hip.  Every operation is one IEEE fp64 operation, and the sums that the definition orders are accumulated in
that order: scores over ascending index inside pieces of SCORE_PIECE points with the pieces added in ascending order, the
refit's sums inside runs of REFIT_RUN points with the runs added in ascending order (``np.add.accumulate`` adds from left
to right, one addition per element).  Only the 3 x 3 eigenvector is not the library's operation sequence: it is LAPACK's.
"""
import numpy as np

SCORE_PIECE = 1024       # points per piece of the scoring sum (a constant of the definition, not a launch parameter)
REFIT_RUN = 64           # points per run of the refit's sums (ditto)
DEGENERATE = 0.05        # |e1 x e2| >= DEGENERATE |e1| |e2|

_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def draw(seed, h, n):
    """The triples (len(h), 3) int64 of the hypotheses ``h`` (offset included) among ``n`` points: splitmix64 on 3h+j+1."""
    h = np.atleast_1d(np.asarray(h, dtype=np.uint64))
    out = np.empty((h.shape[0], 3), dtype=np.int64)
    with np.errstate(over="ignore"):
        for j in range(3):
            ctr = np.uint64(3) * h + np.uint64(j + 1)
            z = np.uint64(seed) + _G * ctr
            z = (z ^ (z >> np.uint64(30))) * _M1
            z = (z ^ (z >> np.uint64(27))) * _M2
            z = z ^ (z >> np.uint64(31))
            out[:, j] = (((z >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    return out


def _norm3(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def fix_sign(n):
    """Rows negated unless their component of largest magnitude is positive; ties go to the lowest axis."""
    n = np.atleast_2d(np.array(n, dtype=np.float64))
    a = np.abs(n)
    lead = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), n[:, 0], np.where(a[:, 1] >= a[:, 2], n[:, 1], n[:, 2]))
    return np.where((lead < 0.0)[:, None], -n, n)


def planes_of_triples(points, tri):
    """(planes (H, 6) = (n, a) with zeros where the triangle is degenerate, ok (H,) bool) of the triples (H, 3)."""
    p0, p1, p2 = points[tri[:, 0]], points[tri[:, 1]], points[tri[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                   e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    ln = _norm3(cr)
    ok = (ln >= DEGENERATE * _norm3(e1) * _norm3(e2)) & (ln > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = fix_sign(cr / ln[:, None])
    planes = np.where(ok[:, None], np.concatenate([n, p0], axis=1), 0.0)
    return planes, ok


def build(points, seed, n_hyp, offset=0):
    """Hypotheses offset .. offset + n_hyp - 1: dict of triples (H, 3), valid (H,) bool and planes (H, 6)."""
    tri = draw(seed, np.arange(offset, offset + n_hyp, dtype=np.uint64), points.shape[0])
    planes, ok = planes_of_triples(points, tri)
    valid = ok & (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    return {"triples": tri, "valid": valid, "planes": np.where(valid[:, None], planes, 0.0)}


def distances(points, planes):
    """Signed distances (H, N): (n_x (x - a_x) + n_y (y - a_y)) + n_z (z - a_z)."""
    pl = np.atleast_2d(planes)
    return (pl[:, 0, None] * (points[None, :, 0] - pl[:, 3, None]) + pl[:, 1, None] * (points[None, :, 1] - pl[:, 4, None])) \
        + pl[:, 2, None] * (points[None, :, 2] - pl[:, 5, None])


def normal_lengths(normals):
    """|m| as it is taken once at upload."""
    return _norm3(normals)


def inliers(points, planes, tau, normals=None, cos_theta=None):
    """(inlier (H, N) bool, dist (H, N))."""
    pl = np.atleast_2d(planes)
    d = distances(points, pl)
    inl = np.abs(d) <= tau
    if cos_theta is not None:
        ln = normal_lengths(normals)
        dot = (pl[:, 0, None] * normals[None, :, 0] + pl[:, 1, None] * normals[None, :, 1]) + pl[:, 2, None] * normals[None, :, 2]
        inl &= (ln > 0.0)[None, :] & (np.abs(dot) >= (cos_theta * ln)[None, :])
    return inl, d


def ordered_sum(v):
    """Sum of the columns of v (H, N): ascending inside pieces of SCORE_PIECE, the pieces added in ascending order."""
    total = np.zeros(v.shape[0])
    for c0 in range(0, v.shape[1], SCORE_PIECE):
        piece = np.concatenate([np.zeros((v.shape[0], 1)), v[:, c0:c0 + SCORE_PIECE]], axis=1)
        total = total + np.add.accumulate(piece, axis=1)[:, -1]
    return total


def score(points, planes, valid, tau, normals=None, cos_theta=None):
    """(count (H,) int64 with -1 for an invalid hypothesis, sum (H,) with 0 there, margin: the smallest ||dist| - tau| of a
    valid hypothesis)."""
    n_hyp = planes.shape[0]
    count = np.full(n_hyp, -1, dtype=np.int64)
    total = np.zeros(n_hyp)
    margin = np.inf
    ids = np.nonzero(valid)[0]
    for b0 in range(0, ids.shape[0], 256):
        sel = ids[b0:b0 + 256]
        inl, d = inliers(points, planes[sel], tau, normals, cos_theta)
        margin = min(margin, float(np.min(np.abs(np.abs(d) - tau))))
        count[sel] = inl.sum(axis=1)
        total[sel] = ordered_sum(np.where(inl, d * d, 0.0))  # + 0.0 is exact
    return count, total, margin


def winner(count, total):
    """Index of the largest count, then the smallest sum, then the smallest h; -1 when no hypothesis is valid."""
    ok = np.nonzero(count >= 0)[0]
    if ok.shape[0] == 0:
        return -1
    order = np.lexsort((ok, total[ok], -count[ok]))
    return int(ok[order[0]])


def refit_sums(points, plane, inl):
    """The ten sums (k, s (3), xx, xy, xz, yy, yz, zz) of q = x - a over the inliers: ascending inside runs of REFIT_RUN
    consecutive points, the runs added in ascending order."""
    n = points.shape[0]
    q = points - plane[3:6]
    cols = [np.ones(n), q[:, 0], q[:, 1], q[:, 2], q[:, 0] * q[:, 0], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
            q[:, 1] * q[:, 1], q[:, 1] * q[:, 2], q[:, 2] * q[:, 2]]
    v = np.where(inl[None, :], np.stack(cols, axis=0), 0.0)  # + 0.0 is exact
    nruns = -(-n // REFIT_RUN)
    pad = np.zeros((10, nruns * REFIT_RUN))
    pad[:, :n] = v
    runs = np.add.accumulate(np.concatenate([np.zeros((10, nruns, 1)), pad.reshape(10, nruns, REFIT_RUN)], axis=2), axis=2)[:, :, -1]
    return np.add.accumulate(np.concatenate([np.zeros((10, 1)), runs], axis=1), axis=1)[:, -1]


def covariance(t):
    """(c (3,), C (3, 3)) of the ten sums: c = s / k, C_ab = S_ab / k - c_a c_b."""
    c = t[1:4] / t[0]
    m = np.empty((3, 3))
    for (a, b), s in zip(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)), t[4:10]):
        m[a, b] = m[b, a] = s / t[0] - c[a] * c[b]
    return c, m


def refine(points, plane, tau, iters, normals=None, cos_theta=None):
    """``iters`` refits of plane (6,): dict of plane (the last), planes (iters + 1, 6: before every iteration and after the
    last), sums (iters, 10), counts (iters,), gap (iters,: (l1 - l0) / l2 of the covariance, inf where the plane was kept),
    margin (the smallest ||dist| - tau| met)."""
    plane = np.array(plane, dtype=np.float64).reshape(6)
    planes, sums, counts, gaps = [plane.copy()], [], [], []
    margin = np.inf
    for _ in range(iters):
        inl, d = inliers(points, plane, tau, normals, cos_theta)
        margin = min(margin, float(np.min(np.abs(np.abs(d) - tau))))
        t = refit_sums(points, plane, inl[0])
        sums.append(t)
        counts.append(int(inl.sum()))
        gap = np.inf
        if t[0] >= 3.0:
            c, m = covariance(t)
            lam, vec = np.linalg.eigh(m)
            gap = (lam[1] - lam[0]) / lam[2] if lam[2] > 0.0 else 0.0
            plane = np.concatenate([fix_sign(vec[:, 0])[0], plane[3:6] + c])
        gaps.append(gap)
        planes.append(plane.copy())
    return {"plane": plane, "planes": np.array(planes), "sums": np.array(sums).reshape(iters, 10),
            "counts": np.array(counts, dtype=np.int64), "gap": np.array(gaps), "margin": margin}


def classify(points, plane, tau, normals=None, cos_theta=None):
    """(mask (N,) bool, dist (N,), count, sum of dist^2 over the inliers in the order of the score, margin)."""
    inl, d = inliers(points, plane, tau, normals, cos_theta)
    total = float(ordered_sum(np.where(inl, d * d, 0.0))[0])
    return inl[0], d[0], int(inl.sum()), total, float(np.min(np.abs(np.abs(d) - tau)))


def _cos(max_normal_angle):
    return None if max_normal_angle is None else float(np.cos(max_normal_angle))


def segment_plane(points, tau, num_iterations=1000, seed=0, refine_iters=3, normals=None, max_normal_angle=None, offset=0):
    """All stages: dict with the stage results and what ``preprocess.segment_plane`` returns (``plane`` (4,), ``point``,
    ``inliers``, ``mask``, ``distance``, ``fitness``, ``inlier_rmse``, ``hypothesis``, ``n_valid``, ``count``, ``sum``)."""
    cos_theta = _cos(max_normal_angle)
    n = points.shape[0]
    b = build(points, seed, num_iterations, offset)
    count, total, margin = score(points, b["planes"], b["valid"], tau, normals, cos_theta)
    w = winner(count, total)
    out = {"build": b, "counts": count, "sums": total, "score_margin": margin, "hypothesis": w,
           "n_valid": int(b["valid"].sum())}
    if w < 0:
        out.update(plane=None, point=None, inliers=np.zeros(0, dtype=np.int32), mask=np.zeros(n, dtype=bool),
                   distance=np.zeros(n), fitness=0.0, inlier_rmse=0.0, count=0, sum=0.0, refine=None, margin=np.inf)
        return out
    r = refine(points, b["planes"][w], tau, refine_iters, normals, cos_theta)
    mask, d, cnt, sm, margin = classify(points, r["plane"], tau, normals, cos_theta)
    nrm, a = r["plane"][:3], r["plane"][3:]
    out.update(plane=np.concatenate([nrm, [-((nrm[0] * a[0] + nrm[1] * a[1]) + nrm[2] * a[2])]]), point=a,
               inliers=np.nonzero(mask)[0].astype(np.int32), mask=mask, distance=d, fitness=cnt / float(n),
               inlier_rmse=float(np.sqrt(sm / cnt)) if cnt else 0.0, count=int(count[w]), sum=float(total[w]), refine=r,
               final_count=cnt, final_sum=sm, margin=min(margin, r["margin"]))
    return out


def segment_planes(points, tau, max_planes, min_inliers=3, num_iterations=1000, seed=0, refine_iters=3, normals=None,
                   max_normal_angle=None):
    """Repeated ``segment_plane`` on the points still unlabelled (ascending original index), round k with hypothesis offset
    k num_iterations: dict of planes (P, 4), points (P, 3), labels (N,) int32, sizes (P,) int32, n_planes, rounds (the
    ``segment_plane`` result of every round that ran, the rejected last one included)."""
    n = points.shape[0]
    labels = np.full(n, -1, dtype=np.int32)
    left = np.arange(n)
    planes, anchors, sizes, rounds = [], [], [], []
    for k in range(max_planes):
        if left.shape[0] < 3:
            break
        r = segment_plane(np.ascontiguousarray(points[left]), tau, num_iterations, seed, refine_iters,
                          None if normals is None else np.ascontiguousarray(normals[left]), max_normal_angle,
                          k * num_iterations)
        rounds.append(r)
        if r["hypothesis"] < 0 or r["inliers"].shape[0] < min_inliers:
            break
        labels[left[r["mask"]]] = k
        planes.append(r["plane"])
        anchors.append(r["point"])
        sizes.append(r["inliers"].shape[0])
        left = left[~r["mask"]]
    return {"planes": np.array(planes).reshape(-1, 4), "points": np.array(anchors).reshape(-1, 3), "labels": labels,
            "sizes": np.array(sizes, dtype=np.int32), "n_planes": len(planes), "rounds": rounds}
