"""Generalized ICP on the GPU (probreg_amd.icp, csrc/icp.hip) against its restatement (tests/oracle_gicp.py, DESIGN.md section
3.16), stage by stage and end to end.

Covariances from normals, matches, the raw ordered sums (all 30 slots, the ones that depend on the per-pair inverse included),
K, S, n_iter, converged and the correspondences are compared byte for byte: test_oracle_gicp.py shows that no decision of the
loop cases lies within 1e-9 (relative) of its threshold.  A pose after a step gets 8 x the disagreement of the host solves of
the same sums (the restatement's ordered Cholesky against oracle_icp's and lstsq), or 1e-12 where that is larger; a loop gets
n_iter times that.  S at the end of a loop is a function of the final pose: it is asserted exactly, which holds because the
restatement takes the step in the device's operation order and the sines and cosines of the two sides round alike at these
angles (observed: every pose of the stage and loop cases is bit-equal).
"""
import functools

import numpy as np
import pytest

import oracle_gicp as ogi
import oracle_icp as oi
from probreg_amd import synthetic

pytestmark = pytest.mark.gpu


def _icp():
    from probreg_amd import icp
    return icp


# --------------------------------------------------------------------------------------------------------- covariances
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_covariances_from_normals_equal_the_host_mirror(n):
    icp = _icp()
    rng = np.random.default_rng(n)
    pts = rng.uniform(-1.0, 1.0, (n, 3))
    nrm = rng.normal(size=(n, 3)) * rng.uniform(1.0e-3, 1.0e3, (n, 1))  # any length, any sign
    nrm[0] = (0.0, 0.0, -2.0)
    plan = icp.IcpPlan()
    try:
        plan.set_source(pts)
        plan.set_target(pts)
        for eps in (1.0e-3, 0.25, 1.0):
            plan.set_source_covariances(normals=nrm, epsilon=eps)
            plan.set_target_covariances(normals=-nrm, epsilon=eps)
            got = plan.covariances("source")
            assert got.shape == (n, 3, 3) and got.tobytes() == icp.covariances_from_normals(nrm, eps).tobytes()
            assert got.tobytes() == ogi.full(ogi.covariances_from_normals(nrm, eps)).tobytes()
            assert plan.covariances("target").tobytes() == got.tobytes()
        explicit = icp.covariances_from_normals(nrm, 0.5)
        plan.set_target_covariances(explicit)
        assert plan.covariances("target").tobytes() == explicit.tobytes()
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------------------- sums and steps
@functools.lru_cache(maxsize=None)
def _stage_clouds():
    """The clouds of test_icp_gpu's stages with the normals generalized ICP needs on both sides, and a pose of the restatement."""
    _, tgt, tn, _ = synthetic.pt2pl_pair(1500, m=10, seed=5)
    src, sn = synthetic.surface_with_normals(64 * 256 + 1, 11)
    sn = sn.astype(np.float32).astype(np.float64)
    pose = oi.icp(src[:500], tgt, np.inf, max_iteration=2)["pose"]
    cs, ct = ogi.covariances_from_normals(sn), ogi.covariances_from_normals(tn)
    for v in (src, tgt, sn, tn, pose, cs, ct):
        v.setflags(write=False)
    return src, tgt, sn, tn, pose, cs, ct


def _same(got, ref):
    return got[0].dtype == np.int32 and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


@pytest.mark.parametrize("m,r", [(63, np.inf), (64, np.inf), (65, np.inf), (64 * 256 + 1, np.inf), (1200, 0.05)])
def test_sums_to_the_last_bit_and_one_step(m, r):
    src, tgt, sn, tn, pose, cs, ct = _stage_clouds()
    src, sn, cs = src[:m], sn[:m], cs[:m]
    q = oi.moved(src, pose)
    idx, d2 = oi.search(q, tgt, r)
    ref = ogi.sums(pose, q, tgt, cs, ct, idx, d2)
    assert ref[0] == m if np.isinf(r) else 6 < ref[0] < m
    new, status, dis = ogi.step(pose, ref)
    assert status == oi.OK
    icp = _icp()
    plan = icp.IcpPlan()
    try:
        plan.set_target(tgt)
        plan.set_source(src)
        plan.set_source_covariances(normals=sn)
        plan.set_target_covariances(normals=tn)
        plan.set_pose(pose)
        plan.search(r)
        assert _same(plan.matches(), (idx, d2))
        got = plan.sums(icp.GENERALIZED)
        st = plan.state()
        plan.step(icp.GENERALIZED)
        after = plan.state()
    finally:
        plan.close()
    worst = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0e-300)))
    print("m %d: raw sums differ from the restatement by %.3e (relative, worst slot)" % (m, worst))
    assert got.tobytes() == ref.tobytes()
    assert st.count == int(ref[0]) and np.float64(st.sum).tobytes() == np.float64(ref[1]).tobytes()
    assert st.pose.tobytes() == pose.tobytes()
    diff = float(np.max(np.abs(after.pose - new)))
    print("m %d: host solves disagree by %.3e, GPU differs from the restatement by %.3e (same bits: %s)"
          % (m, dis, diff, after.pose.tobytes() == new.tobytes()))
    assert after.status == "ok" and after.n_iter == 1
    assert diff <= oi.step_bound(dis)


def test_steps_that_cannot_be_taken_leave_the_pose():
    _, tgt, _, tn, _, _, ct = _stage_clouds()
    icp = _icp()
    start = oi.pose12(np.eye(3), [1.0e-3, 0.0, -1.0e-3])
    copies = np.tile(tgt[10], (6, 1))
    cases = [(np.concatenate([tgt[:5], tgt[:3] + 50.0]), np.concatenate([tn[:5], tn[:3]]), 5),  # count < 6
             (copies, np.tile(tn[10], (6, 1)), 6)]                                               # six copies of one point
    for src, sn, count in cases:
        ref = ogi.gicp(src, tgt, 0.01, ogi.covariances_from_normals(sn), ct, pose=start)
        assert ref["K"] == count and ref["n_iter"] == 0 and ref["status"] == oi.DEGENERATE
        plan = icp.IcpPlan()
        try:
            plan.set_target(tgt)
            plan.set_source(src)
            plan.set_source_covariances(normals=sn)
            plan.set_target_covariances(normals=tn)
            plan.set_pose(start)
            plan.iterate(icp.GENERALIZED, 0.01)
            st = plan.state()
            assert _same(plan.matches(), (ref["index"], ref["d2"]))
            assert st.pose.tobytes() == start.tobytes() and not st.converged and st.n_iter == 0
            assert st.status == "degenerate" and st.count == count
            plan.search(0.01)
            plan.step(icp.GENERALIZED)
            st = plan.state()
            assert st.pose.tobytes() == start.tobytes() and st.status == "degenerate" and st.n_iter == 0
        finally:
            plan.close()


# ---------------------------------------------------------------------------------------------------------------- loop
def _plan_run(case, chunk, explicit=False):
    src, tgt, sn, tn, r, max_it, _ = case
    icp = _icp()
    plan = icp.IcpPlan()
    try:
        plan.set_target(tgt)
        plan.set_source(src)
        if explicit:
            plan.set_source_covariances(icp.covariances_from_normals(sn))
            plan.set_target_covariances(ogi.covariances_from_normals(tn))  # (n, 6) is taken as well
        else:
            plan.set_source_covariances(normals=sn)
            plan.set_target_covariances(normals=tn)
        plan.iterate(icp.GENERALIZED, r, max_it, chunk=chunk)
        st = plan.state()
        idx, d2 = plan.matches()
        objective = plan.sums(icp.GENERALIZED)[29]
    finally:
        plan.close()
    return (st.pose.tobytes(), st.count, np.float64(st.sum).tobytes(), st.n_iter, st.converged, st.status, idx.tobytes(),
            d2.tobytes(), np.float64(objective).tobytes())


def _result_bytes(res):
    return (res.transformation.rot.tobytes(), res.transformation.t.tobytes(), res.correspondences.tobytes(), res.fitness,
            res.inlier_rmse, res.n_iter, res.converged, res.objective)


@pytest.mark.parametrize("name", ogi.LOOP_CASES)
def test_loop_equals_the_restatement(name):
    case, ref = ogi.loop_case(name, synthetic)
    src, tgt, sn, tn, r, max_it, _ = case
    icp = _icp()
    res = icp.registration_gicp(src, tgt, r, source_normals=sn, target_normals=tn, max_iteration=max_it)
    assert res.n_iter == ref["n_iter"] and res.converged == ref["converged"]
    assert res.correspondences.dtype == np.int32 and res.correspondences.tobytes() == ref["correspondences"].tobytes()
    assert res.fitness == ref["fitness"] and res.correspondences.shape[0] == ref["K"]
    bound = ref["n_iter"] * oi.step_bound(ref["disagreement"])
    diff = float(max(np.max(np.abs(res.transformation.rot - ref["rot"])), np.max(np.abs(res.transformation.t - ref["t"]))))
    print("%s, n_iter %d: host solves disagree by %.3e per step, GPU pose differs by %.3e, rmse by %.3e, objective by %.3e"
          % (name, ref["n_iter"], ref["disagreement"], diff, abs(res.inlier_rmse - ref["inlier_rmse"]),
             abs(res.objective - ref["objective"])))
    assert res.transformation.scale == 1.0 and diff <= bound
    assert abs(res.inlier_rmse - ref["inlier_rmse"]) <= bound
    assert abs(res.objective - ref["objective"]) <= 1.0e-9 * ref["objective"]
    again = icp.registration_gicp(src, tgt, r, source_normals=sn, target_normals=tn, max_iteration=max_it)
    assert _result_bytes(again) == _result_bytes(res)
    runs = [_plan_run(case, chunk) for chunk in (1, 4, max_it)]
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][0] == np.concatenate([res.transformation.rot.reshape(9), res.transformation.t]).tobytes()
    assert runs[0][1] == ref["K"] and runs[0][2] == np.float64(ref["S"]).tobytes()
    assert runs[0][8] == np.float64(res.objective).tobytes()
    fitness, rmse, corr = icp.evaluate_registration(src, tgt, r, res.transformation)
    assert (fitness, rmse) == (res.fitness, res.inlier_rmse) and corr.tobytes() == res.correspondences.tobytes()


def test_explicit_covariances_give_the_same_bytes():
    case, _ = ogi.loop_case("gicp_r0.05", synthetic)
    src, tgt, sn, tn, r, max_it, _ = case
    icp = _icp()
    assert _plan_run(case, 8, explicit=True) == _plan_run(case, 8)
    a = icp.registration_gicp(src, tgt, r, source_normals=sn, target_normals=tn)
    b = icp.registration_gicp(src, tgt, r, source_covariances=icp.covariances_from_normals(sn),
                              target_covariances=icp.covariances_from_normals(tn))

    class Cloud(object):
        def __init__(self, points, normals):
            self.points, self.normals = points, normals

    c = icp.registration_gicp(Cloud(src, sn), Cloud(tgt, tn), r)
    assert _result_bytes(a) == _result_bytes(b) == _result_bytes(c)


def test_estimated_normals_register_the_pair():
    """No normals handed in: both clouds get them from fpfh.FPFH(...).estimate_normals, whose signs are arbitrary."""
    import oracle_global_reg as og

    case, _ = ogi.loop_case("gicp_r0.05", synthetic)
    src, tgt, _, _, r, _, (rot, t) = case
    icp = _icp()
    res = icp.registration_gicp(src, tgt, r, normal_radius=0.15)
    deg, shift = og.pose_error(res.transformation.rot, res.transformation.t, rot, t)
    start = icp.evaluate_registration(src, tgt, r)[0]
    print("estimated normals: n_iter %d, converged %s, fitness %.3f from %.3f, %.4f deg, %.2e"
          % (res.n_iter, res.converged, res.fitness, start, deg, shift))
    # the thresholds test_oracle_icp.py holds point-to-plane to on this pair, with the analytic normals
    assert res.n_iter >= 1 and res.fitness > start and deg < 0.2 and shift < 1.0e-3


def test_missing_covariances_are_an_error():
    case, _ = ogi.loop_case("gicp_r0.05", synthetic)
    src, tgt, sn, tn, r, _, _ = case
    icp = _icp()
    plan = icp.IcpPlan()
    try:
        with pytest.raises(ValueError, match="set the source first"):
            plan.set_source_covariances(normals=sn)
        plan.set_target(tgt, tn)
        plan.set_source(src)
        plan.search(r)
        for call in (lambda: plan.sums(icp.GENERALIZED), lambda: plan.step(icp.GENERALIZED),
                     lambda: plan.iterate(icp.GENERALIZED, r), lambda: plan.covariances("source")):
            with pytest.raises(RuntimeError, match="covariances"):
                call()
        plan.set_source_covariances(normals=sn)
        with pytest.raises(RuntimeError, match="covariances of the target"):
            plan.sums(icp.GENERALIZED)
        plan.set_target_covariances(normals=tn)
        assert plan.sums(icp.GENERALIZED)[0] > 6
        plan.set_source(src)  # a new source drops its covariances
        plan.search(r)
        with pytest.raises(RuntimeError, match="covariances of the source"):
            plan.sums(icp.GENERALIZED)
        plan.set_source_covariances(normals=sn)
        plan.set_target(tgt, tn)  # and a new target the target's
        plan.search(r)
        with pytest.raises(RuntimeError, match="covariances of the target"):
            plan.iterate(icp.GENERALIZED, r)
    finally:
        plan.close()


def test_existing_kinds_do_not_see_the_covariances():
    case, _ = ogi.loop_case("gicp_r0.1", synthetic)
    src, tgt, sn, tn, r, _, _ = case
    icp = _icp()
    out = []
    for with_cov in (False, True):
        plan = icp.IcpPlan()
        try:
            plan.set_target(tgt, tn)
            plan.set_source(src)
            if with_cov:
                plan.set_source_covariances(normals=sn)
                plan.set_target_covariances(normals=tn)
            got = []
            for kind in ("point_to_point", "point_to_plane"):
                plan.set_pose(None)
                plan.search(r)
                got.append(plan.sums(kind).tobytes())
                plan.iterate(kind, r, 30)
                st = plan.state()
                got.append((st.pose.tobytes(), st.count, st.sum, st.n_iter, st.converged, st.status, plan.matches()[0].tobytes()))
            out.append(got)
        finally:
            plan.close()
    assert out[0] == out[1]
    assert out[0][3][3] == oi.loop_case("pt2pl_plane", synthetic)[1]["n_iter"]
