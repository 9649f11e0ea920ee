"""Plane segmentation on the GPU (csrc/plane_seg.hip through probreg_amd.preprocess), stage by stage against the restatement of
tests/oracle_plane.py on the clouds of tests/plane_cases.py.  Triples, flags, hypothesis planes, counts, sums, the winner and
the refit's ten sums are compared bit for bit with no hypothesis or point excused; the refitted planes within the eigenvector
perturbation bound of the FPFH normal tests (|n_gpu - n_ref| <= 1e-13 / gap); masks, inliers, labels and sizes exactly.  The
exact comparisons behind a refit rest on test_oracle_plane.py: no point of these clouds is closer than 1e-4 to the threshold
there, ten orders above that bound.

Measured on one MI355X: the largest fraction of the eigenvector bound reached over the table scene (seeds 0 and 1, with and
without normals), the room's first round, the grid cloud and the truncated clouds is 0.0055; the anchors are equal to the last bit.
"""
import functools

import numpy as np
import pytest

import oracle_plane as op
import plane_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp():
    from probreg_amd import preprocess
    return preprocess


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _plan(pp, pts, nrm=None):
    plan = pp.PlanePlan()
    plan.set_points(pts, nrm)
    return plan


@functools.lru_cache(maxsize=None)
def _cut_result(n, n_hyp):
    return op.segment_plane(np.ascontiguousarray(pc.table_scene()[0][:n]), pc.TAU, n_hyp, 3)


def _stage_cases():
    pts, nrm, _, _ = pc.table_scene()
    cos = float(np.cos(pc.NORMAL_ANGLE))
    cases = {"table0": (pts, None, pc.TAU, None, pc.N_HYP, 0, lambda: pc.table_result(0)),
             "table1": (pts, None, pc.TAU, None, pc.N_HYP, 1, lambda: pc.table_result(1)),
             "table_normals": (pts, nrm, pc.TAU, cos, pc.N_HYP, 0, lambda: pc.table_result(0, True)),
             "room": (pc.room_scene()[0], None, pc.TAU, None, pc.N_HYP, 0, lambda: pc.room_result()["rounds"][0]),
             "grid": (pc.grid_cloud(), None, pc.GRID_TAU, None, pc.GRID_HYP, pc.GRID_SEED, lambda: pc.grid_result(False)),
             "grid_shifted": (pc.grid_cloud() + pc.SHIFT_EXACT, None, pc.GRID_TAU, None, pc.GRID_HYP, pc.GRID_SEED,
                              lambda: pc.grid_result(True))}
    # a lane past the end (H = 257), one hypothesis, one full piece and one point more
    for n, h in ((1024, 257), (1025, 257), (1025, 1), (2248, 1)):
        cases["cut_%d_%d" % (n, h)] = (np.ascontiguousarray(pts[:n]), None, pc.TAU, None, h, 3,
                                       functools.partial(_cut_result, n, h))
    return cases


STAGE_CASES = _stage_cases()


@pytest.mark.parametrize("name", sorted(STAGE_CASES))
def test_every_stage_against_the_restatement(pp, name):
    pts, nrm, tau, cos, n_hyp, seed, want_fn = STAGE_CASES[name]
    want = want_fn()
    plan = _plan(pp, pts, nrm)
    plan.build(seed, n_hyp)
    tri, planes, valid = plan.hypotheses()
    assert np.array_equal(tri, want["build"]["triples"])
    assert np.array_equal(valid, want["build"]["valid"])
    assert _same(planes, want["build"]["planes"])
    plan.score(tau, cos)
    counts, sums = plan.scores()
    assert np.array_equal(counts, want["counts"])
    assert _same(sums, want["sums"])
    idx, n_valid, cnt, sm, plane = plan.best()
    assert (idx, n_valid) == (want["hypothesis"], want["n_valid"])
    if idx < 0:
        plan.close()
        return
    assert cnt == want["count"] and _same(sm, want["sum"]) and _same(plane, want["build"]["planes"][idx])
    # the refits one by one: sums bit for bit, planes within the eigenvector bound
    ref = want["refine"]
    worst = 0.0
    cur = plane
    for it in range(3):
        cur, trace = plan.refine(cur, tau, 1, cos)
        assert int(trace[0, 0]) == ref["counts"][it]
        assert _same(trace[0], ref["sums"][it]), "iteration %d" % it
        if np.isfinite(ref["gap"][it]):
            bound = pc.EIGEN_BOUND / ref["gap"][it]
            worst = max(worst, float(np.max(np.abs(cur - ref["planes"][it + 1]))) / bound)
        else:
            assert _same(cur, ref["planes"][it + 1])  # fewer than three inliers: the plane is kept
        assert _same(cur[3:], ref["planes"][it + 1][3:])  # a + c of equal sums
    print("%s: largest fraction of the eigenvector bound = %.3g" % (name, worst))
    assert worst <= 1.0
    whole, trace = plan.refine(plane, tau, 3, cos)
    assert _same(whole, cur) and _same(trace, ref["sums"])
    mask, dist, k, total = plan.classify(whole, tau, cos)
    assert np.array_equal(mask, want["mask"])
    assert k == want["final_count"] == int(mask.sum())
    assert np.max(np.abs(dist - want["distance"])) <= 4.0 * pc.EIGEN_BOUND / np.min(ref["gap"]) * max(1.0, np.max(np.abs(pts - whole[3:])))
    # the sum of the final squared distances in the score's order, from the device's own distances
    assert _same(total, op.ordered_sum(np.where(mask, dist * dist, 0.0)[None, :])[0])
    plan.close()


@pytest.mark.parametrize("name,seed,normals", [("table", 0, False), ("table", 1, False), ("table", 0, True)])
def test_segment_plane_finds_the_table(pp, name, seed, normals):
    pts, nrm, is_table, _ = pc.table_scene()
    want = pc.table_result(seed, normals)
    kw = dict(normals=nrm, max_normal_angle=pc.NORMAL_ANGLE) if normals else {}
    got = pp.segment_plane(pts, pc.TAU, pc.N_HYP, seed, **kw)
    assert (got.hypothesis, got.n_valid, got.count) == (want["hypothesis"], want["n_valid"], want["count"])
    assert _same(got.sum, want["sum"])
    assert np.array_equal(got.mask, want["mask"]) and np.array_equal(got.inliers, want["inliers"])
    assert got.inliers.dtype == np.int32 and got.mask.dtype == np.bool_
    if normals:  # no point that merely lies within tau of the table joins it
        assert np.array_equal(got.mask, is_table)
    else:
        assert int((got.mask & ~is_table).sum()) == 2
    bound = pc.EIGEN_BOUND / np.min(want["refine"]["gap"])
    assert np.max(np.abs(got.plane[:3] - want["plane"][:3])) <= bound and _same(got.point, want["point"])
    assert abs(got.plane[3] - want["plane"][3]) <= 4.0 * bound * np.max(np.abs(got.point))
    assert got.fitness == want["fitness"] and abs(got.inlier_rmse - want["inlier_rmse"]) <= 1e-12
    assert np.all(np.abs(got.distance[got.mask]) <= pc.TAU)
    again = pp.segment_plane(pts, pc.TAU, pc.N_HYP, seed, **kw)  # the same call twice: equal bytes
    for a, b in zip(got, again):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and (np.asarray(a).dtype.kind != "f" or _same(a, b))


def test_segment_planes_cuts_the_room_and_equals_the_loop(pp):
    pts, part, _ = pc.room_scene()
    want = pc.room_result()
    got = pp.segment_planes(pts, pc.TAU, 4, pc.ROOM_MIN_INLIERS, pc.N_HYP, 0)
    assert got.n_planes == 3 and got.sizes.tolist() == [1500, 900, 500] and got.sizes.dtype == np.int32
    assert np.array_equal(got.labels, want["labels"]) and np.array_equal(got.labels, part) and got.labels.dtype == np.int32
    assert np.array_equal(got.sizes, want["sizes"])
    for k in range(3):
        bound = pc.EIGEN_BOUND / np.min(want["rounds"][k]["refine"]["gap"])
        assert np.max(np.abs(got.planes[k, :3] - want["planes"][k, :3])) <= bound
        assert _same(got.points[k], want["points"][k])
    # the definition: a loop over segment_plane on what is left, GPU against GPU, bit for bit
    left = np.arange(pc.ROOM_N)
    labels = np.full(pc.ROOM_N, -1, dtype=np.int32)
    for k in range(4):
        seg = pp.segment_plane(np.ascontiguousarray(pts[left]), pc.TAU, pc.N_HYP, 0, hypothesis_offset=k * pc.N_HYP)
        if seg.inliers.shape[0] < pc.ROOM_MIN_INLIERS:
            assert k == 3 and seg.inliers.shape[0] == 11
            break
        assert _same(seg.plane, got.planes[k]) and _same(seg.point, got.points[k])
        labels[left[seg.mask]] = k
        left = left[~seg.mask]
    assert np.array_equal(labels, got.labels)
    again = pp.segment_planes(pts, pc.TAU, 4, pc.ROOM_MIN_INLIERS, pc.N_HYP, 0)
    assert _same(again.planes, got.planes) and _same(again.points, got.points) and np.array_equal(again.labels, got.labels)
    two = pp.segment_planes(pts, pc.TAU, 2, pc.ROOM_MIN_INLIERS, pc.N_HYP, 0)
    assert two.n_planes == 2 and _same(two.planes, got.planes[:2])
    assert np.array_equal(two.labels, np.where(got.labels < 2, got.labels, -1))
    none = pp.segment_planes(pts, pc.TAU, 4, 2000, pc.N_HYP, 0)
    assert none.n_planes == 0 and none.planes.shape == (0, 4) and np.all(none.labels == -1)


def test_remove_keeps_the_rest_in_ascending_index(pp):
    pts, nrm, _, _ = pc.table_scene()
    want = pc.table_result(0, True)
    plan = _plan(pp, pts, nrm)
    cos = float(np.cos(pc.NORMAL_ANGLE))
    mask, _, _, _ = plan.classify(np.concatenate([want["plane"][:3], want["point"]]), pc.TAU, cos)
    assert plan.remove() == int((~mask).sum()) == plan.count()
    left = np.ascontiguousarray(pts[~mask])
    b = op.build(left, 9, 257, 1000)
    plan.build(9, 257, 1000)
    tri, planes, valid = plan.hypotheses()
    assert np.array_equal(tri, b["triples"]) and np.array_equal(valid, b["valid"]) and _same(planes, b["planes"])
    plan.score(pc.TAU, cos)  # the normals moved with their points
    counts, sums = plan.scores()
    wc, ws, _ = op.score(left, b["planes"], b["valid"], pc.TAU, np.ascontiguousarray(nrm[~mask]), cos)
    assert np.array_equal(counts, wc) and _same(sums, ws)
    plan.close()


def test_planted_hypotheses_and_a_plane_exactly_at_the_threshold(pp):
    pts = pc.quarter_cloud()
    planes = np.array([[0.0, 0.0, 1.0, 0.0, 0.0, 0.0],      # z = 0: the point at z = 0.25 is exactly at tau
                       [0.0, 0.0, 1.0, 7.0, -3.0, 0.5],     # z = 0.5: the point at z = 0.25 alone, exactly at tau
                       [0.0, 0.0, 1.0, 0.0, 0.0, 0.125],
                       [0.0, 0.0, 1.0, 0.0, 0.0, 0.0],      # marked invalid
                       [0.0, 0.0, 1.0, 0.0, 0.0, -0.25]])
    valid = np.array([True, True, True, False, True])
    plan = _plan(pp, pts)
    plan.set_hypotheses(planes, valid)
    plan.score(0.25)
    counts, sums = plan.scores()
    wc, ws, _ = op.score(pts, planes, valid, 0.25)
    assert np.array_equal(counts, wc) and _same(sums, ws)
    assert counts.tolist() == [17, 1, 17, -1, 16]
    assert plan.best()[:3] == (0, 4, 17) and sums[0] == 0.0625 and sums[2] == 0.265625  # 17 inliers twice: the smaller sum
    with pytest.raises(Exception, match="no triples"):
        plan.hypotheses()
    plan.score(np.nextafter(0.25, 0.0))
    assert plan.scores()[0].tolist() == [16, 0, 17, -1, 0]
    mask, dist, k, total = plan.classify(planes[0], 0.25)
    assert k == 17 and mask[16] and dist[16] == 0.25 and total == 0.0625
    plan.close()


def test_exact_clouds(pp):
    r = pp.segment_plane(pc.lattices(), 0.0, 64, 0)
    want = op.segment_plane(pc.lattices(), 0.0, 64, 0)
    assert r.hypothesis == want["hypothesis"] == 4 and r.count == 25 and r.sum == 0.0  # count and sum tie: the smaller h
    assert np.array_equal(r.mask, want["mask"]) and np.all(r.distance[r.mask] == 0.0)
    r = pp.segment_plane(pc.quarter_cloud(), 0.25, 64, 0, refine_iters=0)
    assert r.count == 17 and r.mask[16] and abs(r.distance[16]) == 0.25
    r = pp.segment_plane(pc.collinear_cloud(), 0.1, 64, 0)
    assert r.plane is None and r.point is None and r.hypothesis == -1 and r.n_valid == 0
    assert r.inliers.shape == (0,) and not r.mask.any() and r.fitness == 0.0
    assert pp.segment_planes(pc.collinear_cloud(), 0.1, 3).n_planes == 0
    a = pp.segment_plane(pc.grid_cloud(), pc.GRID_TAU, pc.GRID_HYP, pc.GRID_SEED)
    b = pp.segment_plane(pc.grid_cloud() + pc.SHIFT_EXACT, pc.GRID_TAU, pc.GRID_HYP, pc.GRID_SEED)
    assert (a.hypothesis, a.n_valid, a.count) == (b.hypothesis, b.n_valid, b.count) == (166, 252, pc.grid_result(False)["count"])
    assert _same(a.sum, b.sum) and np.array_equal(a.mask, b.mask) and np.array_equal(a.mask, pc.grid_result(False)["mask"])


def test_argument_and_call_order_errors(pp):
    from probreg_amd import _lib

    pts, nrm, _, _ = pc.table_scene()
    plan = pp.PlanePlan()
    with pytest.raises(_lib.ProbregHipError):
        plan.build(0, 16)  # no points
    with pytest.raises(ValueError):
        plan.set_points(pts[:2])
    plan.set_points(pts)
    with pytest.raises(_lib.ProbregHipError):
        plan.score(0.1)  # no hypotheses
    with pytest.raises(ValueError):
        plan.build(0, 0)
    plan.build(0, 16)
    with pytest.raises(_lib.ProbregHipError):
        plan.scores()  # not scored
    with pytest.raises(_lib.ProbregHipError):
        plan.score(0.1, 0.5)  # a normal test without normals
    with pytest.raises(ValueError):
        plan.score(-0.1)
    with pytest.raises(ValueError):
        plan.score(0.1, 1.5)
    with pytest.raises(_lib.ProbregHipError):
        plan.remove()  # nothing classified
    with pytest.raises(ValueError):
        plan.refine(np.full(6, np.nan), 0.1)
    plan.close()
    for kw in (dict(distance_threshold=-1.0), dict(num_iterations=0), dict(max_normal_angle=0.3), dict(points=pts[:, :2])):
        args = dict(points=pts, distance_threshold=0.01)
        args.update(kw)
        with pytest.raises(ValueError):
            pp.segment_plane(**args)
