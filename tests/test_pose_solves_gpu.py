"""The closed-form pose solve (jacobi_svd -> determinant correction on the smallest singular value -> pose) at every call site
on the GPU, on the planar, collinear, mirrored, tied and coincident families of tests/oracle_pose.py: the rigid and affine
M-steps of CPD from explicit arrays, the batched CPD M-step, FilterReg's weighted Kabsch (3-D SVD, 2-D atan2) and its M-step
from explicit arrays, the point-to-point step of ICP, and the three-point hypotheses and the refit of the global registration.

Wherever the rotation is unique its entries are within max(8 K_ref eps cond, 1e-12) of the NumPy restatement (K_ref: the
family's pooled disagreement of two host solves, tests/test_oracle_pose.py prints it) and the translation within that bound
times max(1, |centroid|_inf).  On every family, unique or not: |R R^T - I|_inf and |det R - 1| <= 64 eps, finite entries,
trace(a^T R) within 64 eps s_1 of sum c_i s_i; CPD's scale, sigma2 and q within 1e-12 relative (a sigma2 on the float32-eps
clamp exactly); the moved matched points within 1e-12 of the extent where they lie in the span of the data; on coincident
clouds the identity, bit for bit, and t the difference of the centroids.

The families are exact (integer clouds, dyadic weights): the cross-covariance the device forms equals the restatement's to
the last bit and what is compared is the solve.  Every test prints the measured difference in units of eps cond.

Worst measured difference / (eps cond) per call site on the MI355X (bound: 8 K_ref, with K_ref between 0.3 and 3.5, or the
1e-12 floor, which is 4500 eps):
    CPD rigid M-step (k_mstep)            2.97   full[M=64], P = I, either update_scale
    FilterReg weighted Kabsch, 3-D        2.60   full[M=64]
    FilterReg weighted Kabsch, 2-D        2.09   d2_full[M=64]
    FilterReg M-step from moments         1.88   mirrored_slab[M=64]
    ICP point-to-point step               0.88   mirrored_slab
    global registration, hypotheses       0.01   thin triangle
    global registration, refit            0.29   planar inliers
The host build of the same text (tests/test_pose_host.py, no contraction) measures 2.88 at most: contraction moves last
bits only.  Moved matched points: 8.6e-16 of the extent at most.  Affine b against np.linalg.solve: at most 0.1 of its bound
(planar_noise_1e-5, cond(YPY) = 3e9).

A finding of these tests, fixed in csrc/small_linalg.h: on a rank-1 cross-covariance the two null columns of V came out of
the Jacobi sweeps turned by an angle that round-off decides, and with them the free rotation about the line.  The batched and
the single CPD path, whose moments differ in the last bits, returned rotations 4.2e-3 apart on the collinear problem of
test_batched_cpd_with_degenerate_neighbours (bound 1e-4; t, sigma2 and q agreed to 1e-8).  V is now completed from its good
column as U is; the same problem agrees to 2.6e-16.
"""
import numpy as np
import pytest

import oracle_global_reg as og
import oracle_icp as oi
import oracle_pose as op

pytestmark = pytest.mark.gpu

FAMILIES = sorted(op.FAMILIES)
AFFINE_SINGULAR = ("planar_axis", "planar_oblique", "collinear", "coincident", "d2_collinear")
MOVED_RTOL = 1.0e-12


def _estep(c, kind):
    from probreg_amd import cpd

    mom, (pt1, p1, px), cy, cx = op.cpd_moments(c["src"], c["tgt"], c["p"][kind])
    return mom, cpd.EstepResult(pt1, p1, px, float(p1.sum())), cy, cx


def _check_t(t, t_ref, bound, centroids, what):
    scale = max([1.0] + [float(np.max(np.abs(v))) for v in centroids])
    diff = float(np.max(np.abs(np.asarray(t) - t_ref)))
    print("%-44s |t - t_ref| %.2e (bound %.2e x %.3g)" % (what, diff, bound, scale))
    assert np.all(np.isfinite(t)) and diff <= bound * scale, what


def _check_moved(rot, t, rot_ref, t_ref, pts, what):
    """The moved points R p + t against the restatement's: unique for p in the span of the data whatever R is."""
    got, ref = pts @ np.asarray(rot).T + t, pts @ rot_ref.T + t_ref
    extent = float(np.max(np.abs(ref - ref.mean(axis=0)))) or float(np.max(np.abs(ref))) or 1.0
    diff = float(np.max(np.abs(got - ref)))
    print("%-44s moved points differ by %.2e of the extent" % (what, diff / extent))
    assert diff <= MOVED_RTOL * extent, what


# --------------------------------------------------------------------------------------------------------- CPD, rigid
@pytest.mark.parametrize("update_scale", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_cpd_rigid_mstep_from_explicit_arrays(family, update_scale):
    from probreg_amd import cpd

    worst = op.Worst()
    for c in op.cases(family):
        d = c["d"]
        for kind in op.P_KINDS:
            what = "%s %s scale=%d" % (c["name"], kind, update_scale)
            mom, es, cy, cx = _estep(c, kind)
            res = cpd.RigidCPD._maximization_step(c["src"], c["tgt"], es, None, update_scale)
            tr = res.transformation
            a = op.cpd_cross_covariance(mom, d)
            ref = op.cpd_rigid(mom, d, update_scale)
            assert tr.rot.shape == (d, d) and tr.t.shape == (d,)
            bound = op.check_rotation(tr.rot, a, d, "cpd", family, what, worst, "CPD rigid")
            op.check_scalars(dict(scale=tr.scale, sigma2=res.sigma2, q=res.q), ref, what)
            if not np.any(a):
                assert np.array_equal(tr.rot, np.identity(d)), what
                if not update_scale:  # mu_x = mu_y = 0 in the centred frame: t is the difference of the centroids
                    assert np.array_equal(tr.t, cx - cy), what
            elif op.describe(a, d)["unique"]:
                t_ref = ref["t"] + cx - ref["scale"] * ref["rot"] @ cy
                _check_t(tr.t, t_ref, bound, [mom[1:4] / mom[0], mom[4:7] / mom[0], cx, cy], what)
            else:
                assert np.all(np.isfinite(tr.t)), what
    print("worst: " + worst.report())


# -------------------------------------------------------------------------------------------------------- CPD, affine
def test_cpd_affine_mstep_raises_or_solves_like_the_reference():
    from probreg_amd import cpd

    solved = set()
    for c in op.all_cases():
        d = c["d"]
        for kind in op.P_KINDS:
            what = "%s %s" % (c["name"], kind)
            mom, es, cy, cx = _estep(c, kind)
            if c["base"] in AFFINE_SINGULAR or c["base"] == "d2_coincident":
                with pytest.raises(np.linalg.LinAlgError):
                    op.cpd_affine(mom, d)
                with pytest.raises(np.linalg.LinAlgError):
                    cpd.AffineCPD._maximization_step(c["src"], c["tgt"], es)
                continue
            ref = op.cpd_affine(mom, d)
            res = cpd.AffineCPD._maximization_step(c["src"], c["tgt"], es)
            bound = max(op.MARGIN * ref["disagreement"], op.TOL_FLOOR * ref["cond"])
            diff = float(np.max(np.abs(res.transformation.b - ref["b"])))
            print("%-40s |b - solve| %.2e, solve against lstsq %.2e, cond(YPY) %.2e, bound %.2e"
                  % (what, diff, ref["disagreement"], ref["cond"], bound))
            assert np.all(np.isfinite(res.transformation.b)) and np.all(np.isfinite(res.transformation.t)), what
            assert diff <= bound, what
            solved.add(c["base"])
    assert {"planar_noise_1e-5", "full", "mirrored", "d2_full"} <= solved


# ------------------------------------------------------------------------------------------------------- CPD, batched
def _batch_problems(dim):
    """The families as registration problems: the source multiplied by the scale the family's target carries (its integer
    rotation), both clouds in units of 2^-10 - still exact, so a planar cloud stays planar and a line a line."""
    pick = (("planar_oblique", 0, 5), ("full", 0, 15), ("collinear", 1, 5), ("mirrored", 0, 15)) if dim == 3 else \
        (("d2_collinear", 0, 5), ("d2_full", 0, 5), ("d2_mirrored", 0, 5))
    cs = [(op.cases(f)[i], k) for f, i, k in pick]
    return [c["name"] for c, _ in cs], [c["src"] * k / 1024.0 for c, k in cs], [c["tgt"] / 1024.0 for c, _ in cs]


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("update_scale", [True, False])
def test_batched_cpd_with_degenerate_neighbours(dim, update_scale):
    """One registration_cpd_batch call over planar, collinear and mirrored problems with a healthy one in between: what
    test_batch_agrees_with_a_loop_over_registration_cpd asserts against single registration_cpd calls, and the healthy problem
    has the bits it has alone."""
    from probreg_amd import cpd
    from test_cpd_batch_gpu import _as_ref, _check, _same_bits

    names, srcs, tgts = _batch_problems(dim)
    kw = dict(w=0.1, maxiter=8, tol=-1, update_scale=update_scale)
    res = cpd.registration_cpd_batch(srcs, tgts, "rigid", **kw)
    for i, name in enumerate(names):
        one = cpd.registration_cpd(srcs[i], tgts[i], "rigid", **kw)
        rot = res[i].transformation.rot
        orth, det, finite = op.invariants(rot)
        print("%-28s |RR^T - I| %.1e  |det - 1| %.1e" % (name, orth, det))
        assert finite and orth <= op.ORTHO and det <= op.ORTHO, name
        assert np.isfinite(res[i].sigma2) and np.isfinite(res[i].q), name
        _check("rigid", res[i], _as_ref("rigid", one), "single path, %s" % name)
    alone = cpd.registration_cpd_batch([srcs[1]], [tgts[1]], "rigid", **kw)[0]
    assert _same_bits("rigid", res[1], alone)


@pytest.mark.parametrize("dim", [3, 2])
def test_batched_affine_cpd_with_degenerate_neighbours(dim):
    from probreg_amd import cpd
    from test_cpd_batch_gpu import _as_ref, _check, _same_bits

    names, srcs, tgts = _batch_problems(dim)
    solvable = [i for i, n in enumerate(names) if n.split("[")[0] in ("full", "mirrored", "d2_full", "d2_mirrored")]
    kw = dict(w=0.1, maxiter=8, tol=-1)
    res = cpd.registration_cpd_batch([srcs[i] for i in solvable], [tgts[i] for i in solvable], "affine", **kw)
    for k, i in enumerate(solvable):
        one = cpd.registration_cpd(srcs[i], tgts[i], "affine", **kw)
        _check("affine", res[k], _as_ref("affine", one), "single path, %s" % names[i])
    # a rank-deficient neighbour is named and does not disturb the healthy problem
    with pytest.raises(np.linalg.LinAlgError) as err:
        cpd.registration_cpd_batch(srcs, tgts, "affine", **kw)
    assert "problem 0 " in str(err.value), str(err.value)
    alone = cpd.registration_cpd_batch([srcs[1]], [tgts[1]], "affine", **kw)[0]
    assert _same_bits("affine", res[solvable.index(1)], alone)


# ---------------------------------------------------------------------------------------------------------- FilterReg
@pytest.mark.parametrize("family", FAMILIES)
def test_filterreg_weighted_kabsch(family):
    """filterreg.kabsch on float32 clouds against the fp64 restatement of the same float32 numbers (the clouds are float32
    numbers to begin with).  2-D runs the atan2 form: on d2_mirrored it returns the best proper rotation, as the SVD with its
    correction does, and on d2_coincident atan2(0, 0) = 0, the identity."""
    from probreg_amd import filterreg

    worst = op.Worst()
    ran = 0
    for c in op.cases(family):
        w = op.kabsch_weights(c)
        if w is None:
            continue
        ran += 1
        d, what = c["d"], c["name"]
        model, target = c["src"].astype(np.float32), c["tgt"].astype(np.float32)
        rot, t = filterreg.kabsch(model, target, w)
        hm, mc, tc = op.kabsch_moments(model, target, w)
        bound = op.check_rotation(rot, hm, d, "kabsch", family, what, worst, "FilterReg kabsch %dD" % d)
        rot_ref, t_ref = op.pose(hm, mc, tc, d, "kabsch")
        if not np.any(hm):
            assert np.array_equal(rot, np.identity(d)) and np.array_equal(t, tc - mc), what
        elif op.describe(hm, d)["unique"]:
            _check_t(t, t_ref, bound, [mc, tc], what)
        if op.describe(hm, d)["unique"] or op.exact_rank(hm) < d:
            _check_moved(rot, t, rot_ref, t_ref, c["src"], what)
    # planar_noise_1e-9 has no float32 target: its 2^-30 across the plane is below float32's resolution
    assert ran > 0 or family == "planar_noise_1e-9"
    print("worst: " + worst.report())


@pytest.mark.parametrize("family,index", [("planar_oblique", 0), ("mirrored_slab", 0), ("collinear", 1), ("d2_mirrored", 0)])
def test_filterreg_mstep_from_handcrafted_moments(family, index):
    """RigidFilterReg._maximization_step with m0 = 1, m1 = the partner, w = 0 and sigma2 = 4: every point weighs
    sqrt(m0 / (m0 + 0) / sigma2) = 1/2, the weighted Kabsch of the case, composed with a previous transformation."""
    from probreg_amd import filterreg, transformation as tf

    c = op.cases(family)[index]
    d, m = c["d"], c["src"].shape[0]
    what = "%s M-step" % c["name"]
    rot_p = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])[:d, :d]   # a quarter turn: composes exactly
    t_p = np.array([3.0, -2.0, 5.0])[:d]
    es = filterreg.EstepResult(np.ones(m, np.float32), c["tgt"].astype(np.float32), None, None)
    res = filterreg.RigidFilterReg._maximization_step(c["src"], c["tgt"], es, tf.RigidTransformation(rot_p, t_p), 4.0, 0.0)
    hm, mc, tc = op.kabsch_moments(c["src"], c["tgt"], np.full(m, 0.5))
    dr, dt = op.pose(hm, mc, tc, d, "kabsch")
    rot_ref, t_ref = dr @ rot_p, t_p @ dr.T + dt
    rot, t = res.transformation.rot, res.transformation.t
    # rot = dr rot_p with an exact rot_p: dr = rot rot_p^T is what the solve returned
    bound = op.check_rotation(rot @ rot_p.T, hm, d, "kabsch", family, what, None)
    if op.describe(hm, d)["unique"]:
        assert np.max(np.abs(rot - rot_ref)) <= bound, what
        _check_t(t, t_ref, bound, [mc, tc, t_p], what)
    # the points of the previous transformation's frame that lie in the span of the data: rot_p y + t_p = src
    y = (c["src"] - t_p) @ rot_p
    _check_moved(rot, t, rot_ref, t_ref, y, what)
    assert res.sigma2 == 4.0 and np.isfinite(res.q)


# ---------------------------------------------------------------------------------------------------------------- ICP
def _icp_case(family):
    """(source, target, start pose): the family's clouds where its partners are nearest neighbours at the identity
    (mirrored_slab) or where any matching keeps the rank (planar_oblique, collinear); the tied case starts from the rounded
    rotation of the family, which moves the scaled cube onto its partner up to the residual."""
    if family == "tied":
        c = op.cases("tied")[0]
        nc, n = op.int_rotation(op.QC)
        return c["src"] * float(n), c["tgt"], oi.pose12(nc / float(n), np.zeros(3))
    if family == "collinear":
        # the family's two lines cross: every source point would take the target next to the crossing and the sums would vanish.
        # Two parallel oblique lines instead, the partner a little along the line and a step across it
        a = 8 * np.arange(8) - 28
        b = a + np.array([1, -1, 0, 1, -1, 0, 1, -1])
        u = np.array([1.0, 2.0, 3.0])
        return np.outer(a, u), np.outer(b, u) + np.array([3.0, 0.0, -1.0]), oi.IDENTITY.copy()
    c = op.cases(family)[0]
    return c["src"], c["tgt"], oi.IDENTITY.copy()


@pytest.mark.parametrize("family", ["planar_oblique", "mirrored_slab", "tied", "collinear"])
def test_icp_point_to_point_step(family):
    from probreg_amd import icp

    worst = op.Worst()
    src, tgt, start = _icp_case(family)
    q = oi.moved(src, start)
    idx, d2 = oi.search(q, tgt, np.inf)
    ref = oi.sums(oi.POINT_TO_POINT, q, tgt, None, idx, d2)
    if family in ("mirrored_slab", "tied", "collinear"):
        assert np.array_equal(idx, np.arange(src.shape[0]))  # the partners are the nearest neighbours
    plan = icp.IcpPlan()
    try:
        plan.set_target(tgt)
        plan.set_source(src)
        plan.set_pose(start)
        plan.search(np.inf)
        got_idx, got_d2 = plan.matches()
        got = plan.sums(oi.POINT_TO_POINT)
        plan.step(oi.POINT_TO_POINT)
        after = plan.state()
    finally:
        plan.close()
    assert got_idx.tobytes() == idx.tobytes() and got_d2.tobytes() == d2.tobytes()
    assert got.tobytes() == ref.tobytes()
    assert after.status == "ok"
    cnt = ref[0]
    qc, yc, hm = ref[2:5] / cnt, ref[5:8] / cnt, ref[8:17].reshape(3, 3)
    info = op.describe(hm, 3)
    claims = {"planar_oblique": (2, True), "mirrored_slab": (3, True), "tied": (3, True), "collinear": (1, False)}[family]
    assert (op.exact_rank(hm), info["unique"]) == claims
    if family == "mirrored_slab":
        assert info["c"] == -1.0 and info["sv"][2] < 1.0e-4 * info["sv"][0]
    if family == "tied":
        assert info["sv"][0] - info["sv"][2] <= 64.0 * op.EPS * info["sv"][0]
    # the step's own rotation: new = delta o start, and start is known
    rs, ts = start[:9].reshape(3, 3), start[9:]
    dr_ref, dt_ref = op.pose(hm, qc, yc, 3, "kabsch")
    new_ref = oi.pose12(dr_ref @ rs, dr_ref @ ts + dt_ref)
    rot, t = after.pose[:9].reshape(3, 3), after.pose[9:]
    what = "ICP %s" % family
    if family == "tied":  # start is a rotation to round-off only: check the composed pose, and delta through the optimum
        orth, det, finite = op.invariants(rot)
        assert finite and orth <= op.ORTHO and det <= op.ORTHO
        bound = op.rot_bound(op.k_ref("tied"), info["cond"])
        diff = float(np.max(np.abs(rot - new_ref[:9].reshape(3, 3))))
        print("%-44s diff / (eps cond) = %8.2f" % (what, diff / (op.EPS * info["cond"])))
        worst.note("ICP step", diff / (op.EPS * info["cond"]), what)
        assert diff <= bound
    else:
        bound = op.check_rotation(rot, hm, 3, "kabsch", family, what, worst, "ICP step")
    if info["unique"]:
        _check_t(t, new_ref[9:], bound, [qc, yc], what)
    _check_moved(rot, t, new_ref[:9].reshape(3, 3), new_ref[9:], src, what)
    print("worst: " + worst.report())


# ------------------------------------------------------------------------------------------------ global registration
def _triangle(height, halfbase):
    """Three correspondences, integers: a thin isosceles triangle turned out of the axes and its exact rigid image.  The sines of
    its angles are about height / halfbase at the ends and twice that at the apex."""
    na, nc = op.int_rotation(op.QA)[0], op.int_rotation(op.QC)[0]
    flat = np.array([[0, 0, 0], [2 * halfbase, 0, 0], [halfbase, height, 0]], dtype=np.float64)
    assert not np.any(flat.sum(axis=0) % 3)
    return 15.0 * flat @ na.T, (flat @ na.T) @ nc.T + np.array([700.0, -300.0, 100.0])


@pytest.mark.parametrize("height,halfbase,valid", [(6, 51, True), (3, 306, False)])
def test_global_registration_thin_triangle_hypotheses(height, halfbase, valid):
    """The sines of the triangle's three angles are all at least 2 x kDegenerate = 0.1 (valid) or all at most kDegenerate / 2
    = 0.025 (invalid), whichever vertex a hypothesis starts from."""
    from probreg_amd import global_reg

    worst = op.Worst()
    p, q = _triangle(height, halfbase)
    for i in range(3):
        e1, e2 = p[(i + 1) % 3] - p[i], p[(i + 2) % 3] - p[i]
        sine = np.linalg.norm(np.cross(e1, e2)) / (np.linalg.norm(e1) * np.linalg.norm(e2))
        assert sine >= 2.0 * og.DEGENERATE if valid else sine <= 0.5 * og.DEGENERATE
    ref = og.build(p, q, 7, 64)
    distinct = np.array([len(set(t)) == 3 for t in ref["triples"]])
    assert distinct.sum() >= 6 and np.array_equal(ref["valid"], distinct & valid)
    plan = global_reg.RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.build(7, 64)
        tri, pose, ok = plan.hypotheses()
    finally:
        plan.close()
    assert np.array_equal(tri, ref["triples"]) and np.array_equal(ok, ref["valid"])
    assert np.all(pose[~ok] == 0.0)
    pm, qm = p.sum(axis=0) / 3.0, q.sum(axis=0) / 3.0
    hm = (p - pm).T @ (q - qm)
    assert op.exact_rank(hm) == 2 and op.describe(hm, 3)["unique"]
    rot_ref, t_ref = op.pose(hm, pm, qm, 3, "kabsch")
    for h in np.nonzero(ok)[0]:
        what = "hypothesis %d %s" % (h, tri[h])
        bound = op.check_rotation(pose[h, :9].reshape(3, 3), hm, 3, "kabsch", "planar_oblique", what, worst, "global build")
        _check_t(pose[h, 9:], t_ref, bound, [pm, qm], what)
        _check_moved(pose[h, :9].reshape(3, 3), pose[h, 9:], rot_ref, t_ref, p, what)
    print("worst: " + worst.report())


def test_global_registration_refit_over_a_planar_inlier_set():
    from probreg_amd import global_reg

    worst = op.Worst()
    rng = np.random.default_rng(11)
    na, nc = op.int_rotation(op.QA)[0], op.int_rotation(op.QC)[0]
    flat = op._embed(op._ints(rng, 64, -40, 40, 2)).astype(np.float64)
    half = rng.integers(-3, 4, size=(32, 2))
    noise = op._embed(np.concatenate([half, -half])).astype(np.float64)   # in the plane: the inlier set stays planar
    p = 15.0 * flat @ na.T
    q = ((flat + noise) @ na.T) @ nc.T + np.array([700.0, -300.0, 100.0])
    start = oi.pose12(nc / 15.0, [700.0, -300.0, 100.0])
    tau = 1.0e4
    pose, cnt, sm, inl = None, 0, 0.0, None
    plan = global_reg.RansacPlan()
    try:
        plan.set_correspondences(p, q)
        pose, cnt, sm, inl = plan.refine(start, tau, 1)
    finally:
        plan.close()
    ref_pose, ref_cnt, _, ref_inl, _, fitted = og.refine(p, q, start, tau, 1)
    assert cnt == ref_cnt == 64 and inl.all() and fitted.shape[0] == 64
    pm, qm = p.sum(axis=0) / 64.0, q.sum(axis=0) / 64.0
    hm = (p - pm).T @ (q - qm)
    assert op.exact_rank(hm) == 2
    what = "refit, planar inliers"
    bound = op.check_rotation(pose[:9].reshape(3, 3), hm, 3, "kabsch", "planar_oblique", what, worst, "global refit")
    rot_ref, t_ref = op.pose(hm, pm, qm, 3, "kabsch")
    _check_t(pose[9:], t_ref, bound, [pm, qm], what)
    _check_moved(pose[:9].reshape(3, 3), pose[9:], rot_ref, t_ref, p, what)
    assert np.max(np.abs(pose - ref_pose)) <= bound * max(1.0, float(np.max(np.abs(qm))))
    print("worst: " + worst.report())
