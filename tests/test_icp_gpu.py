"""ICP on the GPU (probreg_amd.icp, csrc/icp.hip, csrc/grid_search.hip) against its restatement (tests/oracle_icp.py), stage
by stage and end to end.

Matches (index and d2), the raw ordered sums, K and S are compared byte for byte: the host tests (test_oracle_icp.py) show that
no decision of the loop cases lies within 1e-9 (relative) of its threshold, and the handcrafted ties are exact.  A pose after
a step gets 8 x the disagreement of two independent host solves of the same sums (SVD against Horn's quaternions, Cholesky
against lstsq), or 1e-12 where that is larger; a loop gets n_iter times that.
"""
import functools

import numpy as np
import pytest

import oracle_global_reg as og
import oracle_icp as oi
from probreg_amd import synthetic

pytestmark = pytest.mark.gpu

EDGES = (None, 0.01, 0.3, 8.0)  # the cloud's own choice, many cells (hashed), a few cells, a single cell
RADII = (0.02, 0.15, np.inf)


def _icp():
    from probreg_amd import icp
    return icp


def _matches(src, tgt, r, pose=None, cell_edge=None):
    plan = _icp().IcpPlan()
    try:
        plan.set_target(tgt, cell_edge=cell_edge)
        plan.set_source(src)
        if pose is not None:
            plan.set_pose(pose)
        plan.search(r)
        return plan.matches()
    finally:
        plan.close()


def _same(got, ref):
    return got[0].dtype == np.int32 and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


# -------------------------------------------------------------------------------------------------------------- search
def test_search_edges():
    q, y = np.array([[0.1, 0.2, 0.3]]), np.array([[0.15, 0.2, 0.3]])
    got = _matches(q, y, 0.1)
    assert got[0][0] == 0 and _same(got, oi.search(q, y, 0.1))
    got = _matches(q, y, 0.01)
    assert got[0][0] == -1 and np.isinf(got[1][0]) and _same(got, oi.search(q, y, 0.01))
    q = synthetic.surface(130, 4)
    for r in (0.7, np.inf):
        assert _same(_matches(q, y, r), oi.search(q, y, r))


def test_search_ties():
    rng = np.random.default_rng(3)
    y = rng.uniform(-1.0, 1.0, (300, 3))
    y[240] = y[7]
    y[23] = y[7]
    q = np.concatenate([y[7:8], y[7:8] + 1.0e-3, rng.uniform(-1.0, 1.0, (70, 3))])
    for edge in EDGES:
        got = _matches(q, y, np.inf, cell_edge=edge)
        assert got[0][0] == 7 and got[0][1] == 7 and got[1][0] == 0.0 and _same(got, oi.search(q, y, np.inf))
    origin = np.zeros((1, 3))
    for y in (np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]), np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])):
        for edge in (None, 0.25, 0.5, 4.0):  # the two targets in cells either side of the query's, and in one cell
            got = _matches(origin, y, np.inf, cell_edge=edge)
            assert got[0][0] == 0 and got[1][0] == 1.0


def test_search_radius_edge_is_inside_and_one_ulp_out_is_not():
    origin, r = np.zeros((1, 3)), 5.0 / 16.0
    y = np.array([[3.0, 4.0, 0.0]]) / 16.0
    for edge in (None, 0.1, 1.0):
        got = _matches(origin, y, r, cell_edge=edge)
        assert got[0][0] == 0 and got[1][0] == r * r
        out = y.copy()
        out[0, 1] = np.nextafter(out[0, 1], np.inf)
        got = _matches(origin, out, r, cell_edge=edge)
        assert got[0][0] == -1 and np.isinf(got[1][0])


@functools.lru_cache(maxsize=None)
def _grid_case(variant):
    src, tgt, (rot, t, _) = synthetic.rigid_pair(1500, m=1200, seed=3)
    src, tgt = src.copy(), tgt.copy()
    if variant == "outlier":
        tgt[700] = (1.0e6, -1.0e6, 1.0e6)
    if variant == "far":
        src[:50, 0] += 3.0 * (tgt[:, 0].max() - tgt[:, 0].min())
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt, oi.pose12(rot, t)


@pytest.mark.parametrize("at_true_pose", [False, True])
@pytest.mark.parametrize("variant", ["plain", "outlier", "far"])
def test_search_does_not_depend_on_the_grid(variant, at_true_pose):
    src, tgt, true_pose = _grid_case(variant)
    pose = true_pose if at_true_pose else oi.IDENTITY
    for r in RADII:
        ref = oi.search(oi.moved(src, pose), tgt, r)
        if variant == "far":
            assert np.all(ref[0][:50] == -1) if np.isfinite(r) else np.all(ref[0][:50] >= 0)
        for edge in EDGES:
            assert _same(_matches(src, tgt, r, pose, edge), ref), (variant, at_true_pose, r, edge)


def _grid_of(tgt):
    plan = _icp().IcpPlan()
    try:
        plan.set_target(tgt)
        return plan.grid()
    finally:
        plan.close()


@pytest.mark.parametrize("case", ["copies_8", "copies_8_large", "quantised", "quantised_fine_edge"])
def test_repeated_and_quantised_targets_get_a_sane_grid(case):
    """No cell edge separates copies of a point: the edge must stop where the distinct points are apart, the levels must reach
    the box, and the matches stay the restatement's (ties between copies go to the smaller index)."""
    base = synthetic.surface(2500 if case == "copies_8_large" else 400, 21)
    src = synthetic.surface(300, 22) + 0.01
    cell_edge = None
    if case.startswith("copies"):
        tgt = np.ascontiguousarray(np.tile(base, (8, 1)))  # 20 000 rows in the large case: more than the edge's sample
    else:
        tgt = np.ascontiguousarray(np.round(synthetic.surface(20000, 21), 1))
        cell_edge = 1.0e-13 if case == "quantised_fine_edge" else None
    extent = float(np.max(tgt.max(axis=0) - tgt.min(axis=0)))
    if cell_edge is None:
        edge, dims, _, levels = _grid_of(tgt)
        print("%s: extent %.3g, cell edge %.4g, %s cells, %d levels" % (case, extent, edge, dims, levels))
        assert extent / 1000.0 < edge <= extent and levels <= 6
    for r in (0.05, np.inf):
        ref = oi.search(src, tgt, r)
        got = _matches(src, tgt, r, cell_edge=cell_edge)
        assert _same(got, ref), (case, r)
    if case.startswith("copies"):
        assert np.all(ref[0] < base.shape[0])  # the first copy wins every tie


def test_far_query_and_far_outlier_without_a_radius():
    """A target point at 1e6 and queries far from every target, searched with no limit (the default of nearest_neighbour):
    the levels reach the box, so the search ends after a few shells per level."""
    _, tgt, _ = _grid_case("outlier")
    q = np.array([[400.0, -300.0, 250.0], [5.0e5, -5.0e5, 5.0e5], [-2.0e6, 0.0, 0.0], [0.1, 0.1, 0.1]])
    assert _same(_icp().nearest_neighbour(q, tgt), oi.search(q, tgt, np.inf))


class _Affine(object):
    """Stands for any result of the library that is not a rigid pose: it only has ``transform``."""

    def __init__(self, b, t):
        self.b, self.t = b, t

    def transform(self, points):
        return points @ self.b.T + self.t


def test_evaluate_registration_takes_any_transformation():
    from probreg_amd.transformation import RigidTransformation

    src, tgt, pose = _grid_case("plain")
    rot, t = pose[:9].reshape(3, 3), pose[9:]
    icp = _icp()
    for tf, moved in ((_Affine(1.02 * rot, t), src @ (1.02 * rot).T + t),
                      (RigidTransformation(rot, t, 1.02), RigidTransformation(rot, t, 1.02).transform(src))):
        ref = oi.evaluate(np.ascontiguousarray(moved), tgt, oi.IDENTITY, 0.05)
        fitness, rmse, corr = icp.evaluate_registration(src, tgt, 0.05, tf)
        assert 0.0 < fitness < 1.0 and fitness == ref["fitness"] and rmse == ref["inlier_rmse"]
        assert corr.tobytes() == oi.correspondences(ref["index"]).tobytes()
    ref = oi.evaluate(src, tgt, pose, 0.05)
    fitness, rmse, corr = icp.evaluate_registration(src, tgt, 0.05, RigidTransformation(rot, t, 1.0))
    assert fitness == ref["fitness"] and rmse == ref["inlier_rmse"] and corr.tobytes() == oi.correspondences(ref["index"]).tobytes()


# ------------------------------------------------------------------------------------------------------- sums and steps
@functools.lru_cache(maxsize=None)
def _stage_clouds():
    _, tgt, nrm, _ = synthetic.pt2pl_pair(1500, m=10, seed=5)
    src = synthetic.surface(64 * 256 + 1, 11)
    pose = oi.icp(src[:500], tgt, np.inf, max_iteration=2)["pose"]  # a pose of the restatement, handed in
    for v in (src, tgt, nrm, pose):
        v.setflags(write=False)
    return src, tgt, nrm, pose


@pytest.mark.parametrize("kind", [oi.POINT_TO_POINT, oi.POINT_TO_PLANE])
@pytest.mark.parametrize("m,r", [(63, np.inf), (64, np.inf), (65, np.inf), (64 * 256 + 1, np.inf), (1200, 0.05)])
def test_sums_to_the_last_bit_and_one_step(m, r, kind):
    src, tgt, nrm, pose = _stage_clouds()
    src = src[:m]
    q = oi.moved(src, pose)
    idx, d2 = oi.search(q, tgt, r)
    ref = oi.sums(kind, q, tgt, nrm, idx, d2)
    assert ref[0] == m if np.isinf(r) else 6 < ref[0] < m
    new, status, dis = oi.step(kind, pose, ref)
    assert status == oi.OK
    plan = _icp().IcpPlan()
    try:
        plan.set_target(tgt, nrm)
        plan.set_source(src)
        plan.set_pose(pose)
        plan.search(r)
        assert _same(plan.matches(), (idx, d2))
        got = plan.sums(kind)
        st = plan.state()
        plan.step(kind)
        after = plan.state()
    finally:
        plan.close()
    assert got.tobytes() == ref.tobytes()
    assert st.count == int(ref[0]) and np.float64(st.sum).tobytes() == np.float64(ref[1]).tobytes()
    assert st.pose.tobytes() == pose.tobytes()
    diff = float(np.max(np.abs(after.pose - new)))
    print("kind %d m %d: host solves disagree by %.3e, GPU differs from the restatement by %.3e" % (kind, m, dis, diff))
    assert after.status == "ok" and after.n_iter == 1
    assert diff <= oi.step_bound(dis)


def test_steps_that_cannot_be_taken_leave_the_pose():
    rng = np.random.default_rng(1)
    tgt = rng.uniform(-1.0, 1.0, (40, 3))
    nrm = rng.normal(size=(40, 3))
    flat = np.tile([0.0, 0.0, 1.0], (40, 1))
    start = oi.pose12(og.rotation_about((1.0, 2.0, 3.0), 1.0e-3), [1.0e-3, 0.0, -1.0e-3])
    cases = [(np.concatenate([tgt[:2], tgt[:3] + 50.0]), None, oi.POINT_TO_POINT, 0.01, 2, "too_few_matches"),
             (np.concatenate([tgt[:5], tgt[:3] + 50.0]), nrm, oi.POINT_TO_PLANE, 0.01, 5, "degenerate"),
             (tgt.copy(), flat, oi.POINT_TO_PLANE, 0.1, 40, "degenerate")]
    for src, normals, kind, r, count, status in cases:
        ref = oi.icp(src, tgt, r, kind, normals, pose=start)
        assert ref["K"] == count and ref["n_iter"] == 0 and oi.correspondences(ref["index"]).shape[0] == count
        plan = _icp().IcpPlan()
        try:
            plan.set_target(tgt, normals)
            plan.set_source(src)
            plan.set_pose(start)
            plan.iterate(kind, r)
            st = plan.state()
            assert _same(plan.matches(), (ref["index"], ref["d2"]))
            assert st.pose.tobytes() == start.tobytes() and not st.converged and st.n_iter == 0
            assert st.status == status and st.count == count
            plan.search(r)
            plan.step(kind)
            st = plan.state()
            assert st.pose.tobytes() == start.tobytes() and st.status == status and st.n_iter == 0
        finally:
            plan.close()


# ---------------------------------------------------------------------------------------------------------------- loop
def _plan_run(case, chunk):
    src, tgt, nrm, kind, r, max_it, _ = case
    plan = _icp().IcpPlan()
    try:
        plan.set_target(tgt, nrm)
        plan.set_source(src)
        plan.iterate(kind, r, max_it, chunk=chunk)
        st = plan.state()
        idx, d2 = plan.matches()
    finally:
        plan.close()
    return st.pose.tobytes(), st.count, np.float64(st.sum).tobytes(), st.n_iter, st.converged, st.status, idx.tobytes(), d2.tobytes()


def _check_loop(res, ref, true_pose=None):
    """The discrete results equal the restatement's; pose and rmse within n_iter step bounds."""
    assert res.n_iter == ref["n_iter"] and res.converged == ref["converged"]
    assert res.correspondences.dtype == np.int32 and res.correspondences.tobytes() == ref["correspondences"].tobytes()
    assert res.fitness == ref["fitness"]
    bound = max(ref["n_iter"], 1) * oi.step_bound(ref["disagreement"])
    diff = float(max(np.max(np.abs(res.transformation.rot - ref["rot"])), np.max(np.abs(res.transformation.t - ref["t"]))))
    print("n_iter %d: host solves disagree by %.3e per step, GPU pose differs by %.3e, rmse by %.3e"
          % (ref["n_iter"], ref["disagreement"], diff, abs(res.inlier_rmse - ref["inlier_rmse"])))
    assert res.transformation.scale == 1.0 and diff <= bound
    assert abs(res.inlier_rmse - ref["inlier_rmse"]) <= bound


@pytest.mark.parametrize("name", oi.LOOP_CASES)
def test_loop_equals_the_restatement(name):
    case, ref = oi.loop_case(name, synthetic)
    src, tgt, nrm, kind, r, max_it, _ = case
    icp = _icp()
    est = "point_to_plane" if kind == oi.POINT_TO_PLANE else "point_to_point"
    res = icp.registration_icp(src, tgt, r, estimation=est, target_normals=nrm, max_iteration=max_it)
    _check_loop(res, ref)
    again = icp.registration_icp(src, tgt, r, estimation=est, target_normals=nrm, max_iteration=max_it)
    assert again.transformation.rot.tobytes() == res.transformation.rot.tobytes()
    assert again.transformation.t.tobytes() == res.transformation.t.tobytes()
    assert again.correspondences.tobytes() == res.correspondences.tobytes()
    assert (again.fitness, again.inlier_rmse, again.n_iter, again.converged) == (res.fitness, res.inlier_rmse, res.n_iter,
                                                                                 res.converged)
    runs = [_plan_run(case, chunk) for chunk in (1, 4, max_it)]
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][0] == np.concatenate([res.transformation.rot.reshape(9), res.transformation.t]).tobytes()
    fitness, rmse, corr = icp.evaluate_registration(src, tgt, r, res.transformation)
    assert (fitness, rmse) == (res.fitness, res.inlier_rmse) and corr.tobytes() == res.correspondences.tobytes()


def test_nearest_neighbour_equals_the_matches_of_a_plan():
    src, tgt, _ = _grid_case("plain")
    for r in (0.15, None):
        got = _icp().nearest_neighbour(src, tgt, r)
        assert _same(got, _matches(src, tgt, np.inf if r is None else r))
        assert _same(got, oi.search(src, tgt, np.inf if r is None else r))


# ------------------------------------------------------------------------------------------------------------ pipeline
def test_global_registration_then_icp():
    from probreg_amd import global_reg

    src, tgt, rot, t = og.family_f_clouds(1)
    start = global_reg.registration_global(src, tgt, max_distance=0.08)
    res = _icp().registration_icp(src, tgt, 0.08, init=start.transformation)
    ref = oi.icp(src, tgt, 0.08, pose=oi.pose12(start.transformation.rot, start.transformation.t))
    assert ref["gap_second"] > oi.GAP and ref["gap_r"] > oi.GAP
    _check_loop(res, ref)
    before = og.pose_error(start.transformation.rot, start.transformation.t, rot, t)
    after = og.pose_error(res.transformation.rot, res.transformation.t, rot, t)
    print("start pose: %.3f deg, %.4f; after ICP (%d steps): %.3f deg, %.4f" % (before + (res.n_iter,) + after))
    assert after[0] <= before[0] and after[1] <= before[1]
