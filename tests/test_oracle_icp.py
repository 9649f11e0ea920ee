"""The NumPy restatement of ICP (tests/oracle_icp.py) on the host: its brute-force search against
SciPy's kd-tree, the decision gaps that allow the GPU tests to demand exact equality, and the outcomes of the loop cases."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import oracle_global_reg as og
import oracle_icp as oi
from probreg_amd import synthetic


def _clouds():
    src, tgt, (rot, t, _) = synthetic.rigid_pair(1500, m=1200, seed=3)
    return src, tgt, oi.pose12(rot, t)


@pytest.mark.parametrize("at_true_pose", [False, True])
@pytest.mark.parametrize("r", [0.02, 0.15, np.inf])
def test_brute_force_search_equals_the_kd_tree(at_true_pose, r):
    src, tgt, true_pose = _clouds()
    q = oi.moved(src, true_pose if at_true_pose else oi.IDENTITY)
    idx, d2 = oi.search(q, tgt, r)
    dist, near = cKDTree(tgt).query(q, k=2)
    clear = dist[:, 0] != dist[:, 1]  # where the tree's own best and second best differ
    assert clear.sum() > 1000
    exact = ((tgt[near[:, 0]] - q) ** 2)
    exact = (exact[:, 0] + exact[:, 1]) + exact[:, 2]
    inside = exact <= r * r
    assert np.array_equal(idx[clear & inside], near[clear & inside, 0])
    assert np.all(idx[clear & ~inside] == -1) and np.all(np.isinf(d2[idx < 0]))
    assert np.array_equal(d2[clear & inside], exact[clear & inside])
    if np.isinf(r):
        assert np.all(idx >= 0)


def test_search_ties_and_the_radius_edge():
    q = np.zeros((1, 3))
    for y in (np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]]), np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])):
        assert oi.search(q, y, np.inf)[0][0] == 0
    y = np.array([[0.5, 0.5, 0.5], [0.25, 0.0, 1.0], [0.25, 0.0, 1.0]])
    assert oi.search(np.array([[0.25, 0.0, 1.0]]), y, 1.0)[0][0] == 1
    edge = np.array([[3.0, 4.0, 0.0]]) / 16.0
    idx, d2 = oi.search(q, edge, 5.0 / 16.0)
    assert idx[0] == 0 and d2[0] == (5.0 / 16.0) ** 2
    out = edge.copy()
    out[0, 1] = np.nextafter(out[0, 1], np.inf)
    idx, d2 = oi.search(q, out, 5.0 / 16.0)
    assert idx[0] == -1 and np.isinf(d2[0])


def test_ordered_sum_follows_the_runs():
    rng = np.random.default_rng(0)
    v = rng.normal(size=(200, 2))
    keep = rng.uniform(size=200) < 0.7
    want = np.zeros(2)
    for r0 in range(0, 200, oi.RUN):
        s = np.zeros(2)
        for m in range(r0, min(r0 + oi.RUN, 200)):
            if keep[m]:
                s = s + v[m]
        want = want + s
    assert np.array_equal(oi.ordered_sum(v, keep), want)


@pytest.mark.parametrize("name", oi.LOOP_CASES)
def test_decision_gaps_of_the_loop_cases(name):
    """No query of the restatement's whole trajectory has its best and second-best d2, or its best d2 and r r, within 1e-9
    (relative): a second implementation in IEEE arithmetic takes the same matches."""
    _, res = oi.loop_case(name, synthetic)
    print("%s: gap_second %.3e gap_r %.3e" % (name, res["gap_second"], res["gap_r"]))
    assert res["gap_second"] > oi.GAP and res["gap_r"] > oi.GAP


def test_loop_outcome_point_to_plane():
    case, res = oi.loop_case("pt2pl_plane", synthetic)
    deg, shift = og.pose_error(res["rot"], res["t"], *case[6])
    print("pt2pl_plane: n_iter %d, %.4f deg, %.2e" % (res["n_iter"], deg, shift))
    assert res["converged"] and res["n_iter"] < 10 and res["status"] == oi.OK
    assert deg < 0.2 and shift < 1.0e-3


def test_loop_outcome_point_to_point_with_outliers():
    case, res = oi.loop_case("filterreg_point", synthetic)
    deg, _ = og.pose_error(res["rot"], res["t"], *case[6])
    print("filterreg_point: n_iter %d, %.4f deg" % (res["n_iter"], deg))
    assert res["converged"] and res["n_iter"] <= 50


def test_loop_outcome_wide_radius_does_not_converge_in_30():
    _, res = oi.loop_case("rigid_point", synthetic)
    assert not res["converged"] and res["n_iter"] == 30 and res["fitness"] == 1.0


def test_steps_that_cannot_be_taken():
    rng = np.random.default_rng(1)
    tgt = rng.uniform(-1.0, 1.0, (40, 3))
    src2 = np.concatenate([tgt[:2] + 0.001, tgt[:3] + 50.0])
    res = oi.icp(src2, tgt, 0.01, oi.POINT_TO_POINT)
    assert res["K"] == 2 and res["n_iter"] == 0 and not res["converged"] and res["status"] == oi.TOO_FEW
    assert np.array_equal(res["pose"], oi.IDENTITY)
    nrm = rng.normal(size=(40, 3))
    src5 = np.concatenate([tgt[:5] + 0.001, tgt[:3] + 50.0])
    res = oi.icp(src5, tgt, 0.01, oi.POINT_TO_PLANE, nrm)
    assert res["K"] == 5 and res["status"] == oi.DEGENERATE and not res["converged"]
    flat = np.tile([0.0, 0.0, 1.0], (40, 1))
    res = oi.icp(tgt + 0.001, tgt, 0.1, oi.POINT_TO_PLANE, flat)
    assert res["K"] == 40 and res["status"] == oi.DEGENERATE and res["n_iter"] == 0
    assert np.array_equal(res["pose"], oi.IDENTITY)
