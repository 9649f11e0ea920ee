"""Plain fp64 NumPy restatement of the closed-form pose solve every rigid method of the library ends in (a d x d
cross-covariance -> SVD -> determinant correction on the smallest singular value -> pose), an independent second solve
(Horn's unit quaternions in 3-D, the atan2 form in 2-D), the affine solve of CPD, and the families of small clouds on which
the solve is rank deficient, mirrored or tied.  No GPU, nothing of csrc/ is read.

Two conventions are in use.  With a = sum P (x - mu_x)(y - mu_y)^T = U S V^T, CPD takes rot = U diag(c) V^T ("cpd": rows of
a are target axes).  With hm = sum (p - pm)(q - qm)^T = U S V^T, Kabsch / ICP / the global registration take
rot = V diag(c) U^T ("kabsch": rows of hm are source axes).  Either maximises trace(a^T rot) resp. trace(rot hm) over proper
rotations; the maximum is sum c_i s_i with c = (1, .., 1, sign det).

The clouds are exact by construction: integer coordinates (times a power of two) that are float32 numbers, an unweighted
mean of exactly zero, rotations n R with integer entries (from an integer quaternion) and weights that are small multiples
of 1/16 summing to a power of two.  Every moment sum of such a case is exact in fp64 in any order of summation, so the
restatement, a host build of the device text and the GPU see the same cross-covariance to the last bit, a planar cloud gives
a cross-covariance of exact rank 2, and what differs between them is the solve alone.

Every family but ``coincident`` leaves a residual (noise inside the span of the data, a mirror, a scale that cannot be
fitted): sigma2 and q of an exact fit are the round-off of a cancellation and no two correct solves agree on them to 1e-12.
"""
import functools
from fractions import Fraction

import numpy as np

from oracle import cpd_numpy as co

EPS = 2.0 ** -52
EPS32 = float(np.finfo(np.float32).eps)
RANK_RULE = 1.0e-14    # jacobi_svd keeps a column whose norm is above RANK_RULE times the largest one
PIVOT_RULE = 1.0e-12   # mstep_body calls an affine pivot below PIVOT_RULE max |YPY| singular
UNIQUE = 1.0e-6        # the rotation is taken as unique while s_{d-1} + c s_d > UNIQUE s_1
TOL_FLOOR = 1.0e-12
MARGIN = 8.0           # the project's margin on the disagreement of two host solves (oracle_global_reg.solve_bound)


# ------------------------------------------------------------------------------------------------------------- solves
def _proper(u, vt):
    return 1.0 if np.linalg.det(u @ vt) >= 0.0 else -1.0


def describe(a, d):
    """sv (descending), c (the determinant correction), cond = s_1 / (s_{d-1} + c s_d), unique, optimum = sum c_i s_i."""
    a = np.asarray(a, dtype=np.float64)[:d, :d]
    u, s, vt = np.linalg.svd(a)
    c = _proper(u, vt)
    den = s[d - 2] + c * s[d - 1]
    unique = bool(s[0] > 0.0 and den > UNIQUE * s[0])
    cond = float(s[0] / den) if den > 0.0 else np.inf
    return {"sv": s, "c": c, "cond": cond, "unique": unique, "optimum": float(np.sum(s[:d - 1]) + c * s[d - 1])}


def rotation_svd(a, d, convention):
    a = np.asarray(a, dtype=np.float64)[:d, :d]
    u, _, vt = np.linalg.svd(a)
    cdiag = np.ones(d)
    cdiag[-1] = _proper(u, vt)
    rot = (u * cdiag) @ vt
    return rot if convention == "cpd" else rot.T


def rotation_second(a, d, convention):
    """The independent solve, written for hm (kabsch); the cpd rotation of a is its transpose."""
    s = np.asarray(a, dtype=np.float64)[:d, :d]
    if d == 2:
        ang = np.arctan2(s[0, 1] - s[1, 0], s[0, 0] + s[1, 1])
        rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    else:
        n = np.array([[s[0, 0] + s[1, 1] + s[2, 2], s[1, 2] - s[2, 1], s[2, 0] - s[0, 2], s[0, 1] - s[1, 0]],
                      [s[1, 2] - s[2, 1], s[0, 0] - s[1, 1] - s[2, 2], s[0, 1] + s[1, 0], s[2, 0] + s[0, 2]],
                      [s[2, 0] - s[0, 2], s[0, 1] + s[1, 0], -s[0, 0] + s[1, 1] - s[2, 2], s[1, 2] + s[2, 1]],
                      [s[0, 1] - s[1, 0], s[2, 0] + s[0, 2], s[1, 2] + s[2, 1], -s[0, 0] - s[1, 1] + s[2, 2]]])
        _, vec = np.linalg.eigh(n)
        w, x, y, z = vec[:, 3]
        rot = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
    return rot.T if convention == "cpd" else rot


def optimum_of(a, rot, d, convention):
    """trace(a^T rot) (cpd) or trace(rot hm) (kabsch): what the rotation is chosen to maximise."""
    a = np.asarray(a, dtype=np.float64)[:d, :d]
    rot = np.asarray(rot, dtype=np.float64)[:d, :d]
    return float(np.sum(a * rot)) if convention == "cpd" else float(np.sum(a * rot.T))


def pose(a, mu_a, mu_b, d, convention, solve=rotation_svd):
    """(rot, t): the proper rotation of the cross-covariance and t = mu_b - rot mu_a, with mu_a the centroid of the cloud that
    moves (CPD's source, Kabsch's model) and mu_b that of the cloud it moves onto."""
    rot = solve(a, d, convention)
    return rot, np.asarray(mu_b, dtype=np.float64)[:d] - rot @ np.asarray(mu_a, dtype=np.float64)[:d]


def invariants(rot):
    """(|R R^T - I|_inf, |det R - 1|, finite)."""
    rot = np.asarray(rot, dtype=np.float64)
    d = rot.shape[0]
    return float(np.max(np.abs(rot @ rot.T - np.identity(d)))), abs(float(np.linalg.det(rot)) - 1.0), bool(np.all(np.isfinite(rot)))


def rot_bound(k_ref, cond):
    return max(MARGIN * k_ref * EPS * cond, TOL_FLOOR)


# ------------------------------------------------------------------------------------------------------- exact helpers
def _frac_matrix(a):
    return [[Fraction(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def exact_rank(a):
    """Rank of the fp64 matrix ``a`` in exact rational arithmetic."""
    m = _frac_matrix(a)
    rows, cols, rank = len(m), len(m[0]), 0
    for c in range(cols):
        piv = next((r for r in range(rank, rows) if m[r][c] != 0), None)
        if piv is None:
            continue
        m[rank], m[piv] = m[piv], m[rank]
        for r in range(rank + 1, rows):
            f = m[r][c] / m[rank][c]
            m[r] = [x - f * y for x, y in zip(m[r], m[rank])]
        rank += 1
    return rank


def exact_det(a):
    m = _frac_matrix(a)
    if len(m) == 2:
        return m[0][0] * m[1][1] - m[0][1] * m[1][0]
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def sv_ratios(a, d):
    """s_k / s_1 for k = 2 .. d of the fp64 matrix, where a ratio below 1e-8 is taken from exact arithmetic (the exact rank,
    and |det| / (s_1 .. s_{d-1}) for the last one) so that it can be told from the SVD's own round-off of about 1e-16."""
    a = np.asarray(a, dtype=np.float64)[:d, :d]
    s = np.linalg.svd(a, compute_uv=False)
    if s[0] == 0.0:
        return [0.0] * (d - 1)
    rank = exact_rank(a)
    out = []
    for k in range(1, d):
        r = float(s[k] / s[0])
        if k >= rank:
            r = 0.0
        elif k == d - 1 and r < 1.0e-8:
            r = abs(float(exact_det(a))) / float(np.prod(s[:d - 1])) / float(s[0])
        out.append(r)
    return out


# ------------------------------------------------------------------------------------------------------------ CPD side
def cpd_moments(src, tgt, p):
    """(moments (32,) of include/probreg_hip.h, (pt1, p1, px)) of the centred clouds as the library stores them (float32) under
    the posterior matrix p (M x N)."""
    src = np.asarray(src, dtype=np.float64)
    tgt = np.asarray(tgt, dtype=np.float64)
    p1, pt1, px = p.sum(axis=1), p.sum(axis=0), p @ tgt
    cy, cx = src.mean(axis=0), tgt.mean(axis=0)
    ys = (src - cy).astype(np.float32).astype(np.float64)
    xs = (tgt - cx).astype(np.float32).astype(np.float64)
    mom = co.moments_from_estep(ys, xs, (pt1, p1, px - np.outer(p1, cx), float(p1.sum())))
    return mom, (pt1, p1, px), cy, cx


def cpd_cross_covariance(mom, d):
    mu_y = mom[4:7] / mom[0]
    return (mom[7:16].reshape(3, 3) - np.outer(mom[1:4], mu_y))[:d, :d]


def cpd_ypy(mom, d):
    mu_y = mom[4:7] / mom[0]
    syy = np.array([[mom[16], mom[17], mom[18]], [mom[17], mom[19], mom[20]], [mom[18], mom[20], mom[21]]])
    return (syy - mom[0] * np.outer(mu_y, mu_y))[:d, :d]


def cpd_rigid(mom, d, update_scale, solve=rotation_svd):
    """dict(rot, t, scale, sigma2, q) of the rigid M-step on the moment block (centred frame).  The scalars are the formulas of
    oracle.cpd_numpy.mstep_from_moments with trace(a^T rot) taken from ``solve``'s rotation."""
    if solve is rotation_svd:
        r = co.mstep_from_moments("rigid", mom, d, update_scale)
        return dict(rot=r.params["rot"], t=r.params["t"], scale=r.params["scale"], sigma2=r.sigma2, q=r.q)
    s0 = mom[0]
    a, ypy = cpd_cross_covariance(mom, d), cpd_ypy(mom, d)
    mu_x, mu_y = mom[1:1 + d] / s0, mom[4:4 + d] / s0
    rot = solve(a, d, "cpd")
    tr_atr, tr_y = np.float64(optimum_of(a, rot, d, "cpd")), np.float64(np.trace(ypy))
    tr_x = mom[22] - s0 * float(mu_x @ mu_x)
    scale = tr_atr / tr_y if update_scale else 1.0
    sigma2 = (tr_x - scale * tr_atr) / (s0 * d) if update_scale else (tr_x + tr_y - scale * tr_atr) / (s0 * d)
    sigma2 = max(sigma2, EPS32)
    q = (tr_x - 2.0 * scale * tr_atr + scale ** 2 * tr_y) / (2.0 * sigma2) + d * s0 * 0.5 * np.log(sigma2)
    return dict(rot=rot, t=mu_x - scale * rot @ mu_y, scale=scale, sigma2=sigma2, q=q)


def affine_pivots(ypy):
    """|pivots| of Gaussian elimination with partial pivoting on ypy^T, relative to max |ypy| (what PIVOT_RULE is applied to)."""
    m = np.array(ypy, dtype=np.float64).T
    d = m.shape[0]
    top = float(np.max(np.abs(m)))
    if top == 0.0:
        return [0.0] * d
    out = []
    for c in range(d):
        r = c + int(np.argmax(np.abs(m[c:, c])))
        m[[c, r]] = m[[r, c]]
        out.append(abs(float(m[c, c])) / top)
        if m[c, c] == 0.0:
            out.extend([0.0] * (d - 1 - c))
            break
        for k in range(c + 1, d):
            m[k] -= m[k, c] / m[c, c] * m[c]
    return out


def cpd_affine(mom, d):
    """dict(b, t, sigma2, q, disagreement) of the affine M-step, or the reference's LinAlgError where ypy is singular: an exact
    rank below d, or a pivot below PIVOT_RULE.  disagreement: np.linalg.solve against np.linalg.lstsq on the same system."""
    ypy = cpd_ypy(mom, d)
    if exact_rank(ypy) < d or min(affine_pivots(ypy)) <= PIVOT_RULE:
        raise np.linalg.LinAlgError("Singular matrix")
    r = co.mstep_from_moments("affine", mom, d)
    a = cpd_cross_covariance(mom, d)
    other = np.linalg.lstsq(ypy.T, a.T, rcond=None)[0].T
    return dict(b=r.params["b"], t=r.params["t"], sigma2=r.sigma2, q=r.q,
                disagreement=float(np.max(np.abs(other - r.params["b"]))), cond=float(np.linalg.cond(ypy)))


# ----------------------------------------------------------------------------------------------------- Kabsch moments
def kabsch_moments(model, target, weight):
    """(hm, model centroid, target centroid) of the weighted Kabsch of cc/kabsch.cc: centroids weighted by w, the covariance by
    w^2 about them, divided by sum w^2."""
    model, target, w = (np.asarray(v, dtype=np.float64) for v in (model, target, weight))
    mc, tc = (w @ model) / w.sum(), (w @ target) / w.sum()
    w2 = w * w
    return ((model - mc).T * w2) @ (target - tc) / w2.sum(), mc, tc


# ----------------------------------------------------------------------------------------------------------- families
def int_rotation(quat):
    """(n R, n): the integer matrix of the rotation of the integer quaternion (w, x, y, z), n = |quat|^2."""
    w, x, y, z = (int(v) for v in quat)
    m = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], dtype=np.int64)
    return m, w * w + x * x + y * y + z * z


QA, QB, QC = (2, 1, 2, 0), (1, 2, 0, 2), (3, 1, 2, 1)   # n = 9, 9, 15
ROT2 = np.array([[3, -4], [4, 3]], dtype=np.int64)      # 5 x the plane rotation by atan2(4, 3)
MIRROR = np.diag([1, 1, -1]).astype(np.int64)


def _zero_sum(v):
    """The same integer rows with the last one replaced by minus the sum of the others: the mean is exactly zero."""
    v = np.array(v, dtype=np.int64)
    v[-1] = -v[:-1].sum(axis=0)
    return v


def _ints(rng, m, lo, hi, cols):
    return _zero_sum(rng.integers(lo, hi + 1, size=(m, cols)))


def _embed(v2):
    return np.column_stack([v2, np.zeros(v2.shape[0], dtype=np.int64)])


def _dense_p(rng, m):
    """M x M positive multiples of 1/16 whose sum is a power of two, so that every moment sum and both weighted centroids of
    an integer cloud are exact: 1/16 or 2/16 off the diagonal, 1/2 and more on it (the partner keeps most of the weight, as in
    a late E-step)."""
    k = rng.integers(1, 3, size=(m, m))
    k[np.arange(m), np.arange(m)] = rng.integers(8, 16, size=m)
    total = int(k.sum())
    for j in rng.integers(0, m, size=(1 << total.bit_length()) - total):
        k[j, j] += 1
    return k / 16.0


def _clouds(family, m, rng):
    """Integer (src, tgt, d) of one family; tgt_i is the partner of src_i."""
    na, nb, nc = int_rotation(QA)[0], int_rotation(QB)[0], int_rotation(QC)[0]
    if family == "full":
        src = _ints(rng, m, -64, 64, 3)
        return src, src @ nc.T + _ints(rng, m, -400, 400, 3), 3        # noise about 25 % of n |src|
    if family in ("planar_axis", "planar_oblique"):
        s2 = _ints(rng, m, -8, 8, 2)
        t2 = s2 @ ROT2.T + _ints(rng, m, -12, 12, 2)                   # in-plane noise
        if family == "planar_axis":
            return _embed(s2), _embed(t2), 3
        return _embed(s2) @ na.T, _embed(t2) @ nb.T, 3
    if family == "mirrored":
        src = _ints(rng, m, -1, 1, 3) * np.array([64, 24, 8]) + _ints(rng, m, -4, 4, 3)
        return src, _zero_sum(src @ MIRROR @ nc.T + _ints(rng, m, -40, 40, 3)), 3
    if family == "mirrored_slab":
        # distinct (x, y) on a coarse grid, z = +-1: relative thickness about 1e-3, the mirror image is the nearest point
        xy = np.array([(128 * (i % 8) - 448, 64 * (i // 8) - 224) for i in range(m)], dtype=np.int64)
        src = np.column_stack([xy, np.where(np.arange(m) % 2 == 0, 1, -1)])
        assert m == 64 and not src.sum(axis=0).any()
        # in-plane noise well below the grid spacing (a residual, see the module docstring), antisymmetric so that it sums to zero
        half = rng.integers(-20, 21, size=(m // 2, 2))
        noise = np.column_stack([np.concatenate([half, -half]), np.zeros(m, dtype=np.int64)])
        return src @ na.T, (src @ MIRROR + noise) @ na.T, 3
    if family in ("tied", "tied_mirrored"):
        assert m in (4, 8)
        cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.int64)
        src = cube if m == 8 else cube[[7, 4, 2, 1]]                   # all corners, or the tetrahedron of alternate ones
        turn = nc @ MIRROR if family == "tied_mirrored" else nc
        tgt = src @ turn.T
        if m == 8:  # a residual that leaves the cross-covariance alone: sum s_i = 0 and sum s_i y_i = 0 for s_i = x y z
            tgt = tgt + np.outer(cube.prod(axis=1), [3, -2, 5])
        if m == 4:
            # four points and a similarity: an exact fit whatever is added (sum f_i y_i^T = 0 only for a shift).  Kept small, so
            # that sigma2 sits on the float32-eps clamp for either update_scale and q is its logarithm term to round-off
            return src / 1024.0, tgt / 1024.0, 3
        return src * 4, tgt * 4, 3
    if family == "collinear":
        a = _ints(rng, m, -8, 8, 1)[:, 0]
        b = _zero_sum((5 * a + rng.integers(-6, 7, size=m))[:, None])[:, 0]
        return np.outer(a, [1, 2, 3]), np.outer(b, [2, -3, 1]), 3
    if family == "coincident":
        return np.tile([3, -5, 2], (m, 1)), np.tile([-7, 1, 4], (m, 1)), 3
    if family == "d2_full":
        src = _ints(rng, m, -64, 64, 2)
        return src, src @ ROT2.T + _ints(rng, m, -100, 100, 2), 2
    if family == "d2_collinear":
        a = _ints(rng, m, -8, 8, 1)[:, 0]
        b = _zero_sum((5 * a + rng.integers(-6, 7, size=m))[:, None])[:, 0]
        return np.outer(a, [1, 2]), np.outer(b, [2, -3]), 2
    if family == "d2_mirrored":
        src = _ints(rng, m, -1, 1, 2) * np.array([64, 16]) + _ints(rng, m, -4, 4, 2)
        return src, _zero_sum(src @ np.diag([1, -1]) @ ROT2.T + _ints(rng, m, -30, 30, 2)), 2
    if family == "d2_coincident":
        return np.tile([3, -5], (m, 1)), np.tile([-7, 1], (m, 1)), 2
    raise KeyError(family)


def _noisy_plane(m, rng, tiny):
    """The oblique plane with noise across it: the source in-plane integers + 2^-16 x integers across (about 2e-5 relative, a
    float32 cloud), the target the same with its noise across multiplied by ``tiny``."""
    na, nb = int_rotation(QA)[0], int_rotation(QB)[0]
    s2 = _ints(rng, m, -4, 4, 2)
    t2 = s2 @ ROT2.T + _ints(rng, m, -6, 6, 2)
    es = _zero_sum(rng.integers(2, 7, size=(m, 1)) * rng.choice([-1, 1], size=(m, 1)))
    et = _zero_sum(rng.integers(16, 49, size=(m, 1)) * rng.choice([-1, 1], size=(m, 1)))
    src = np.column_stack([s2 * 65536, es]).astype(np.float64) @ na.T
    tgt = np.column_stack([(t2 * 65536).astype(np.float64), et * tiny]) @ nb.T
    # in units of 2^-16: in-plane coordinates of a few tens, so that a translation can be held to 1e-12 at all
    return src / 65536.0, tgt / 65536.0, 3


# family -> ((M, ...), claimed rank of the cross-covariance, sign of its determinant (0: none), unique)
FAMILIES = {
    "full": ((64, 8), 3, 1, True),
    "planar_axis": ((8,), 2, 0, True),
    "planar_oblique": ((8, 3), 2, 0, True),
    "planar_noise_1e-5": ((8,), 3, None, True),
    "planar_noise_1e-9": ((8,), 3, None, True),   # rank 3 as real numbers, rank 2 to jacobi_svd's 1e-14 rule
    "mirrored": ((64, 8), 3, -1, True),
    "mirrored_slab": ((64,), 3, -1, True),
    "tied": ((8, 4), 3, 1, True),
    "tied_mirrored": ((8, 4), 3, -1, False),
    "collinear": ((4, 8), 1, 0, False),
    "coincident": ((4,), 0, 0, False),
    "d2_full": ((64, 3), 2, 1, True),
    "d2_collinear": ((4,), 1, 0, True),
    "d2_mirrored": ((8,), 2, -1, True),
    "d2_coincident": ((4,), 0, 0, False),
    "scaled": ((0,), None, None, True),
}
SCALED_BASES = ("full", "planar_oblique", "mirrored")
# 2^40 and 2^-40 on the base clouds read in units of 2^-12 (integers of a few hundred to a few thousand: an extent of about 1),
# which keeps the entries of every scaled cross-covariance within about 2^-84 .. 2^80, far inside jacobi_svd's supported range
SCALES = (2.0 ** 28, 2.0 ** -52)
P_KINDS = ("identity", "dense")


def _seed(family, m):
    return 1000 * (sorted(FAMILIES).index(family) + 1) + m


@functools.lru_cache(maxsize=None)
def _base(family, m):
    rng = np.random.default_rng(_seed(family, m))
    if family.startswith("planar_noise"):
        src, tgt, d = _noisy_plane(m, rng, 1.0 if family.endswith("1e-5") else 2.0 ** -30)
    else:
        src, tgt, d = _clouds(family, m, rng)
    if family in ("tied", "tied_mirrored", "coincident", "d2_coincident"):
        # a uniform background plus the diagonal keeps sum P x y^T a multiple of sum x_i y_i^T (the clouds sum to zero, or are
        # one point each); coincident clouds give a = 0 under any weights
        dense = (np.full((m, m), 1.0) + 13.0 * np.identity(m)) / 16.0
    else:
        dense = _dense_p(rng, m)
    return np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64), d, dense


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family, read-only: dict(name, family, base, d, src, tgt, p: {"identity", "dense"}, scale)."""
    out = []
    if family == "scaled":
        todo = [(b, FAMILIES[b][0][0], s) for b in SCALED_BASES for s in SCALES]
    else:
        todo = [(family, m, 1.0) for m in FAMILIES[family][0]]
    for base, m, scale in todo:
        src, tgt, d, dense = _base(base, m)
        c = {"name": "%s[M=%d%s]" % (base, m, "" if scale == 1.0 else ",x2^%d" % (int(np.log2(scale)) + 12)), "family": family,
             "base": base, "d": d, "src": src * scale, "tgt": tgt * scale, "scale": scale,
             "p": {"identity": np.identity(m), "dense": dense}}
        for v in (c["src"], c["tgt"], c["p"]["identity"], c["p"]["dense"]):
            v.setflags(write=False)
        out.append(c)
    return tuple(out)


def claims(case):
    """(rank, sign, unique) the family claims of this case's cross-covariance."""
    return FAMILIES[case["base"]][1:]


def all_cases(families=None):
    return [c for f in (families or sorted(FAMILIES)) for c in cases(f)]


def case_matrices(case):
    """Every cross-covariance a call site forms of this case: (label, a, d, convention)."""
    out = []
    for kind in P_KINDS:
        mom = cpd_moments(case["src"], case["tgt"], case["p"][kind])[0]
        out.append(("cpd/" + kind, cpd_cross_covariance(mom, case["d"]), case["d"], "cpd"))
    w = kabsch_weights(case)
    if w is not None:
        out.append(("kabsch", kabsch_moments(case["src"], case["tgt"], w)[0], case["d"], "kabsch"))
    return out


def kabsch_weights(case):
    """Positive float32 weights for the weighted Kabsch of this case, or None where its clouds are no float32 numbers or M is no
    power of two.  All 1/2: the weighted centroids stay exactly zero and sum w^2 = M / 4 is a power of two, so hm is exact."""
    for v in (case["src"], case["tgt"]):
        if not np.array_equal(v.astype(np.float32).astype(np.float64), v):
            return None
    m = case["src"].shape[0]
    return np.full(m, 0.5, dtype=np.float32) if m & (m - 1) == 0 else None


@functools.lru_cache(maxsize=None)
def k_ref(family):
    """The family's pooled host disagreement: the largest |R_svd - R_second| / (eps cond) over every cross-covariance of its
    cases whose rotation is unique (0 where none is)."""
    worst = 0.0
    for c in cases(family):
        for _, a, d, conv in case_matrices(c):
            info = describe(a, d)
            if info["unique"]:
                diff = float(np.max(np.abs(rotation_svd(a, d, conv) - rotation_second(a, d, conv))))
                worst = max(worst, diff / (EPS * info["cond"]))
    return worst


def nominal_ratios(case, kind):
    """s_k / s_1 (k = 2 .. d) of the CPD cross-covariance of the case as a matrix of rational numbers: the clouds as stored
    (float32, centred) under the weights, formed without any rounding.  What the construction places next to RANK_RULE; the
    fp64 matrix a call site forms adds its own round-off of about 1e-16 to a ratio that is smaller than that."""
    d, p = case["d"], case["p"][kind]
    ys = (case["src"] - case["src"].mean(axis=0)).astype(np.float32).astype(np.float64)
    xs = (case["tgt"] - case["tgt"].mean(axis=0))
    fr = lambda arr: [[Fraction(float(v)) for v in row] for row in arr]
    yf, xf, pf = fr(ys), fr(xs), fr(p)
    m, n = len(yf), len(xf)
    s0 = sum(pf[i][j] for i in range(m) for j in range(n))
    p1 = [sum(pf[i]) for i in range(m)]
    pt1 = [sum(pf[i][j] for i in range(m)) for j in range(n)]
    mu_y = [sum(p1[i] * yf[i][k] for i in range(m)) / s0 for k in range(d)]
    mu_x = [sum(pt1[j] * xf[j][k] for j in range(n)) / s0 for k in range(d)]
    px = [[sum(pf[i][j] * (xf[j][k] - mu_x[k]) for j in range(n)) for k in range(d)] for i in range(m)]
    a = [[sum(px[i][r] * (yf[i][c] - mu_y[c]) for i in range(m)) for c in range(d)] for r in range(d)]
    af = np.array([[float(v) for v in row] for row in a])
    s = np.linalg.svd(af, compute_uv=False)
    if s[0] == 0.0:
        return [0.0] * (d - 1)
    det = a[0][0] * a[1][1] - a[0][1] * a[1][0] if d == 2 else (
        a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) - a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0])
        + a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]))
    out = [float(v / s[0]) for v in s[1:]]
    if out[-1] < 1.0e-8:
        out[-1] = abs(float(det)) / float(np.prod(s[:d - 1])) / float(s[0])
    if d == 3 and out[0] < 1.0e-8:  # rank 1 or below: the 2 x 2 minors decide
        minors = max(abs(a[i][j] * a[k][l] - a[i][l] * a[k][j]) for i in range(3) for k in range(i + 1, 3)
                     for j in range(3) for l in range(j + 1, 3))
        out[0] = float(minors) / float(s[0]) ** 2
    return out


# ------------------------------------------------------------------------------------------------------------- checks
ORTHO = 64.0 * EPS     # |R R^T - I|_inf, |det R - 1| and the optimum (times s_1) of any solve
SCALAR_RTOL = 1.0e-12  # scale, sigma2, q: independent of the free choice of a non-unique rotation


class Worst(object):
    """The largest measured (difference from the restatement) / (eps cond) per call site, for the record."""

    def __init__(self):
        self.ratio = {}

    def note(self, site, ratio, what):
        if ratio > self.ratio.get(site, (-1.0, ""))[0]:
            self.ratio[site] = (ratio, what)

    def report(self):
        return "; ".join("%s %.2f (%s)" % (k, v[0], v[1]) for k, v in sorted(self.ratio.items()))


def check_rotation(rot, a, d, convention, family, what, worst=None, site=""):
    """Everything a rotation of the cross-covariance ``a`` must satisfy: the invariants and the optimum always, the entries
    against the SVD restatement where the rotation is unique.  Returns the bound the entries were (or would be) held to."""
    rot = np.asarray(rot, dtype=np.float64)[:d, :d]
    info = describe(a, d)
    orth, det, finite = invariants(rot)
    assert finite, "%s: non-finite rotation" % what
    assert orth <= ORTHO and det <= ORTHO, "%s: |RR^T - I| = %.2e, |det - 1| = %.2e (allowed %.2e)" % (what, orth, det, ORTHO)
    opt = optimum_of(a, rot, d, convention)
    assert abs(opt - info["optimum"]) <= ORTHO * info["sv"][0], \
        "%s: optimum %.17g against %.17g, s1 = %.3e" % (what, opt, info["optimum"], info["sv"][0])
    if not info["unique"]:
        print("%-44s not unique: invariants and optimum only (|RR^T - I| %.1e)" % (what, orth))
        return TOL_FLOOR
    bound = rot_bound(k_ref(family), info["cond"])
    diff = float(np.max(np.abs(rot - rotation_svd(a, d, convention))))
    ratio = diff / (EPS * info["cond"])
    print("%-44s diff / (eps cond) = %8.2f   (diff %.2e, cond %.2e, bound %.2e)" % (what, ratio, diff, info["cond"], bound))
    if worst is not None:
        worst.note(site, ratio, what)
    assert diff <= bound, "%s: rotation differs by %.3e, bound %.3e" % (what, diff, bound)
    return bound


def check_scalars(got, ref, what):
    """scale, sigma2, q of a rigid M-step: 1e-12 relative; a sigma2 on the float32-eps clamp must be exact."""
    for k in ("scale", "sigma2", "q"):
        print("%-44s %-6s %.17g against %.17g" % (what, k, got[k], ref[k]))
        if np.isnan(ref["scale"]):
            # 0 / 0: the scale of two coincident clouds.  Nothing that follows from it is defined (the reference's Python
            # max(nan, eps) and the device's fmax already differ on sigma2)
            assert np.isnan(got["scale"]), "%s: scale %.17g, the reference has NaN" % (what, got["scale"])
            break
        assert np.isfinite(got[k]), "%s: %s is not finite" % (what, k)
        if k == "sigma2" and ref[k] == EPS32:
            assert got[k] == EPS32, "%s: sigma2 %.17g should sit on the clamp" % (what, got[k])
        else:
            assert abs(got[k] - ref[k]) <= SCALAR_RTOL * abs(ref[k]), "%s: %s %.17g against %.17g" % (what, k, got[k], ref[k])
