"""Deterministic point-cloud families, poses and EM states for the E-step tests that leave the tube-like surface of
probreg_amd.synthetic behind (tests/test_cloud_families.py holds their preconditions on the CPU, tests/test_estep_families_gpu.py
runs every CPD E-step engine on them).  The shapes restate tools/fuzz_fused.py::make_clouds; nothing here needs a GPU.

    volume      uniform sample of the unit cube: no surface anywhere, every block has neighbours on all sides
    aniso       uniform sample of a 10 : 1 : 1 box: long thin kd-tree cells, group / chunk boxes of very different extent per axis
    clusters    two Gaussian blobs of different width 6 units apart: empty space between them, whole blocks without a partner
    lopsided    one blob in the source; a quarter of the TARGET is a second blob 6 units away that the source lacks: column
                blocks with no source point in reach (late: their column sums are exact zeros)

The target is the same sample (another subset when the sizes differ) moved by rot_zx(9, -4) and a small translation, with noise of
0.004, in another order.  Both clouds are float32-representable.  Plain module: no pytest hooks, no fixtures.
"""
from collections import namedtuple

import numpy as np

from oracle import cpd_numpy as co
from probreg_amd.synthetic import rot_zx

FAMILIES = ("volume", "aniso", "clusters", "lopsided")
M_DEFAULT, N_DEFAULT = 8200, 9001   # both >= 8192 (matrix-core engines legal), no multiple of 32 / 128 / 256 / 1024: every last
SEED = 5                            # group, block and chunk is partly padded
FAR = (900.0, -1300.0, 400.0)
BLOB = np.array([6.0, 0.5, -0.3])   # centre of the second cluster
TRUE_MOTION = (9.0, -4.0)           # rot_zx angles of the target's motion
NEAR_POSE = (7.0, -3.0)             # 2 degrees short of it
JUMP_POSE = (12.0, 2.0)             # the pose the state-jump tests hop to (scale 1.05)
JUMP_SCALE = 1.05
SIGMA2_LATE = {"volume": 4e-4, "aniso": 4e-4, "clusters": 4e-4, "lopsided": 2e-3}

State = namedtuple("State", ["lin", "t", "scale", "sigma2"])   # z = scale * lin y + t


def make_clouds(family, m=M_DEFAULT, n=N_DEFAULT, seed=SEED, dim=3, far=None):
    """(source [m, dim], target [n, dim]) of `family` as float64 arrays of float32-representable numbers."""
    assert family in FAMILIES and dim in (2, 3)
    g = np.random.default_rng(seed)
    k = max(m, n)
    if family == "volume":
        base = g.random((k, 3))
    elif family == "aniso":
        base = g.random((k, 3)) * np.array([10.0, 1.0, 1.0])
    elif family == "clusters":
        a = 0.4 * g.standard_normal((k // 2, 3))
        b = 0.15 * g.standard_normal((k - k // 2, 3)) + BLOB
        base = np.concatenate([a, b])[g.permutation(k)]
    else:
        base = 0.4 * g.standard_normal((k, 3))
    src = base[:m].copy()
    tgt = (base[:n] @ rot_zx(*TRUE_MOTION).T + np.array([0.05, -0.03, 0.02]) + 0.004 * g.standard_normal((n, 3)))[g.permutation(n)]
    if family == "lopsided":
        tgt[:n // 4] = 0.15 * g.standard_normal((n // 4, 3)) + BLOB
    if dim == 2:
        src, tgt = src[:, :2].copy(), tgt[:, :2].copy()
    if far is not None:
        off = np.asarray(far, dtype=np.float64)[:dim]
        src, tgt = src + off, tgt + off
    return src.astype(np.float32).astype(np.float64), tgt.astype(np.float32).astype(np.float64)


def dead_columns(family, n):
    """Indices of the target points that belong to the blob the source lacks (none but for `lopsided`)."""
    return np.arange(n // 4) if family == "lopsided" else np.arange(0)


def _rotation(angles, dim):
    # (2-D: the rotation about z alone - the upper 2 x 2 block of rot_zx with a tilt about x is no rotation)
    return rot_zx(*angles) if dim == 3 else rot_zx(angles[0], 0.0)[:2, :2].copy()


def pose(src, tgt, name="near", affine=False):
    """(linear part, t, scale): `near` is 2 degrees short of the true motion at scale 1, `jump` is JUMP_POSE at scale 1.05; t puts
    the moved source's centroid on the target's.  `affine`: a non-orthogonal linear part R diag(1.06, 0.96, 1) + 0.03 e0 e1^T."""
    dim = src.shape[1]
    lin = _rotation(NEAR_POSE if name == "near" else JUMP_POSE, dim)
    scale = 1.0 if name == "near" else JUMP_SCALE
    if affine:
        assert name == "near"
        shear = np.zeros((dim, dim))
        shear[0, 1] = 0.03
        lin = lin @ np.diag([1.06, 0.96, 1.0][:dim]) + shear
    t = tgt.mean(axis=0) - scale * lin @ src.mean(axis=0)
    return lin, t, scale


def sigma2_of(family, state, src, tgt):
    """dense: the registration's own initial sigma2; mid: 0.02 x that; late: 4e-4 (lopsided: 2e-3, see test_cloud_families.py);
    jump: mid / 50; jump_deep: mid / 800."""
    dense = co.squared_kernel_sum_closed_form(src, tgt)
    if state == "dense":
        return dense
    if state == "mid":
        return 0.02 * dense
    if state == "jump":
        return 0.02 * dense / 50.0
    if state == "jump_deep":
        return 0.02 * dense / 800.0
    assert state == "late"
    return SIGMA2_LATE[family]


def make_state(family, state, src, tgt, affine=False):
    lin, t, scale = pose(src, tgt, "jump" if state.startswith("jump") else "near", affine)
    return State(lin, t, scale, sigma2_of(family, state, src, tgt))


def centred(src, tgt):
    """What a plan is given: both clouds centred in fp64, rounded to float32.  Returns (s32, t32, cy, cx)."""
    cy, cx = src.mean(axis=0), tgt.mean(axis=0)
    return (src - cy).astype(np.float32), (tgt - cx).astype(np.float32), cy, cx


def centred_state(st, cy, cx):
    """The same map between the centred clouds: z - cx = s L (y - cy) + t'  with  t' = t + s L cy - cx."""
    return State(st.lin, st.t + st.scale * st.lin @ cy - cx, st.scale, st.sigma2)


def transformed(st, pts):
    return st.scale * np.asarray(pts, dtype=np.float64) @ st.lin.T + st.t


def amplification(tgt, sigma2):
    """mean |x|^2 / (D sigma2) of the centred target: by how much the cancellation in sigma2's numerator amplifies an error of
    the sums (the lean matrix-core row pass runs up to 64, the fused sweep up to 256)."""
    x = np.asarray(tgt, dtype=np.float64)
    x = x - x.mean(axis=0)
    return float(np.mean(np.sum(x * x, axis=1))) / (x.shape[1] * sigma2)


# ----------------------------------------------------------------------------------------------------------------------------
# the cases the GPU file runs (test_cloud_families.py asserts their preconditions with the oracle alone)
# ----------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", ["family", "state", "w", "m", "n", "dim", "far", "affine"])


def case(family, state, w, m=M_DEFAULT, n=N_DEFAULT, dim=3, far=None, affine=False):
    return Case(family, state, float(w), m, n, dim, far, affine)


def grid_cases():
    """family x state x w.  `lopsided` takes w = 0.1 in its dense state only: with the uniform term the blob that has no partner
    keeps less than 0.7 N of the mass afterwards (mid: 0.68 N; late, at sigma2 = 4e-4: 0.09 N)."""
    return [case(f, s, w) for f in FAMILIES for s in ("dense", "mid", "late") for w in (0.0, 0.1)
            if not (f == "lopsided" and s != "dense" and w > 0.0)]


def two_d_cases():
    return [case("clusters", s, 0.0, dim=2) for s in ("dense", "mid", "late")]


def swapped_cases():
    return [case(f, "mid", 0.0 if f == "lopsided" else 0.1, m=N_DEFAULT, n=M_DEFAULT) for f in FAMILIES]


def jump_cases():
    """`jump`: sigma2 50 x below `mid`.  `jump_deep`: 800 x below - a tenth of the columns now have their nearest source point
    beyond the cull radius of the new sigma2 alone (exponents up to 440): only the stale seed widened by the motion keeps them."""
    return [case(f, s, 0.0) for f in ("clusters", "aniso") for s in ("jump", "jump_deep")]


def far_cases():
    return [case(f, "mid", 0.0, far=FAR) for f in ("clusters", "volume")]


def affine_cases():
    return [case(f, "mid", 0.0, affine=True) for f in FAMILIES]


def all_cases():
    return grid_cases() + two_d_cases() + swapped_cases() + jump_cases() + far_cases() + affine_cases()


def case_id(c):
    tag = "%s-%s-w%g" % (c.family, c.state, c.w)
    if (c.m, c.n) != (M_DEFAULT, N_DEFAULT):
        tag += "-%dx%d" % (c.m, c.n)
    if c.dim != 3:
        tag += "-2d"
    if c.far is not None:
        tag += "-far"
    if c.affine:
        tag += "-affine"
    return tag


def case_clouds(c):
    return make_clouds(c.family, c.m, c.n, SEED, c.dim, c.far)


def case_state(c, src, tgt):
    return make_state(c.family, c.state, src, tgt, c.affine)


_SETUP, _ORACLE = {}, {}


def case_setup(c):
    """Everything a test needs of a case, computed once: the clouds as generated (src, tgt), the state between them (st), the
    centred float32 clouds a plan is given (s32, t32, their centres cy, cx) and the state between those (st_c)."""
    if c not in _SETUP:
        src, tgt = case_clouds(c)
        st = case_state(c, src, tgt)
        s32, t32, cy, cx = centred(src, tgt)
        _SETUP[c] = dict(src=src, tgt=tgt, st=st, s32=s32, t32=t32, cy=cy, cx=cx, st_c=centred_state(st, cy, cx))
    return _SETUP[c]


def oracle_estep(c):
    """The fp64 C oracle's E-step of a case (cached; callers must not modify it) as an oracle.cpd_numpy.EstepResult.  On exactly
    the float32 values the plan holds, widened to fp64 - so that the kernels' arithmetic is all that differs - except for the
    `far` cases, which go through the registrar's own fp64 centring: those are evaluated on the clouds as generated."""
    if c not in _ORACLE:
        from oracle import cpd_c

        s = case_setup(c)
        if c.far is not None:
            es = cpd_c.expectation_step(transformed(s["st"], s["src"]), s["tgt"], s["st"].sigma2, c.w)
        else:
            es = cpd_c.expectation_step(transformed(s["st_c"], s["s32"].astype(np.float64)), s["t32"].astype(np.float64),
                                        s["st_c"].sigma2, c.w)
        _ORACLE[c] = co.EstepResult(*es)
    return _ORACLE[c]
