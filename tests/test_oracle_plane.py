"""The restatement of plane segmentation (tests/oracle_plane.py) on the clouds of tests/plane_cases.py:
what it finds, how far its decisions are from their thresholds, and that ``segment_planes`` is the loop over ``segment_plane``
that the definition says it is.  The exact comparisons of tests/test_plane_gpu.py rest on the margins pinned here.  No GPU.

Figures of the restatement (this file asserts them):
  table, tau = 0.01, H = 1000: 985 / 988 valid hypotheses for seeds 0 / 1, winners 254 / 658; the best four hypotheses tie at
      1503 inliers, so the sum decides; every refit ends on the 1500 table points and the two outliers that lie 0.002 and
      0.0065 from the table (1502), 0.0204 degrees from the generating normal; the smallest ||dist| - tau| met in the refits
      is 2.6e-4.  With normals and 20 degrees: winner 272, exactly the 1500 table points, margin 2.0e-3.
  room, segment_planes(tau = 0.01, max_planes = 4, min_inliers = 100): 1500, 900, 500 - floor and walls to the point, each
      within 0.03 degrees of its generating normal; the fourth round's 11-point plane is rejected; margins >= 2.3e-3.
"""
import numpy as np
import pytest

import oracle_plane as op
import plane_cases as pc

MARGIN = 1.0e-4


@pytest.mark.parametrize("seed,n_valid,hyp", [(0, 985, 254), (1, 988, 658)])
def test_table_scene(seed, n_valid, hyp):
    pts, _, is_table, normal = pc.table_scene()
    assert pts.shape == (pc.TABLE_N, 3) and int(is_table.sum()) == pc.TABLE_PLANE_N
    r = pc.table_result(seed)
    assert r["n_valid"] == n_valid and r["hypothesis"] == hyp
    order = np.lexsort((np.arange(pc.N_HYP), r["sums"], -r["counts"]))
    assert order[0] == hyp
    assert r["counts"].max() == 1503 and int((r["counts"] == 1503).sum()) >= 4  # a tie of counts: the sum decides
    assert r["sums"][order[0]] < r["sums"][order[1]]
    assert r["count"] == 1503 and r["sum"] == r["sums"][hyp]
    # the points found: the table and the two outliers that lie within tau of it, whatever the seed
    true_dist = (pts - np.array([0.3, -0.2, 0.5])) @ normal
    near = np.abs(true_dist) <= pc.TAU
    assert int(near.sum()) == 1502 and np.array_equal(r["mask"], near)
    assert np.array_equal(r["inliers"], np.nonzero(near)[0]) and r["inliers"].dtype == np.int32
    assert r["refine"]["counts"].tolist() == [1503, 1502, 1502]
    assert r["margin"] > MARGIN
    assert np.all(r["refine"]["gap"] > 0.9)
    assert pc.angle_deg(r["plane"][:3], normal) < 0.03
    assert abs(np.linalg.norm(r["plane"][:3]) - 1.0) < 1e-15
    assert r["plane"][np.argmax(np.abs(r["plane"][:3]))] > 0.0
    assert r["fitness"] == 1502 / 2248.0 and 0.0 < r["inlier_rmse"] < pc.NOISE
    assert np.array_equal(r["distance"], op.distances(pts, np.concatenate([r["plane"][:3], r["point"]]))[0])


def test_table_scene_with_normals():
    """Within 20 degrees of the plane's normal: the two outliers near the table (random normals) do not join."""
    pts, nrm, is_table, normal = pc.table_scene()
    r = pc.table_result(0, True)
    assert r["hypothesis"] == 272 and r["count"] == 1500
    assert np.array_equal(r["mask"], is_table)
    assert r["margin"] > MARGIN
    plain = pc.table_result(0)
    assert int((plain["mask"] & ~is_table).sum()) == 2
    # a zero normal never passes, not even at 90 degrees (cos = 0), where every other normal does
    zero = np.array(nrm)
    zero[r["inliers"][:7]] = 0.0
    inl, _ = op.inliers(pts, np.concatenate([r["plane"][:3], r["point"]]), pc.TAU, zero, 0.0)
    assert int(inl.sum()) == 1502 - 7


def test_room_planes_and_the_loop_over_segment_plane():
    pts, part, normals = pc.room_scene()
    assert pts.shape == (pc.ROOM_N, 3)
    rr = pc.room_result()
    assert rr["n_planes"] == 3 and rr["sizes"].tolist() == [1500, 900, 500]
    assert [x["inliers"].shape[0] for x in rr["rounds"]] == [1500, 900, 500, 11]
    assert all(x["margin"] > MARGIN for x in rr["rounds"])
    assert np.array_equal(rr["labels"], part)
    for k in range(3):
        assert pc.angle_deg(rr["planes"][k, :3], normals[k]) < 0.03
    # segment_planes is the loop over segment_plane on what is left, with offsets k H
    left = np.arange(pc.ROOM_N)
    labels = np.full(pc.ROOM_N, -1, dtype=np.int32)
    for k in range(4):
        r = op.segment_plane(np.ascontiguousarray(pts[left]), pc.TAU, pc.N_HYP, 0, 3, None, None, k * pc.N_HYP)
        assert r["hypothesis"] == rr["rounds"][k]["hypothesis"]
        if r["inliers"].shape[0] < pc.ROOM_MIN_INLIERS:
            assert k == 3
            break
        assert np.array_equal(r["plane"], rr["planes"][k]) and np.array_equal(r["point"], rr["points"][k])
        labels[left[r["mask"]]] = k
        left = left[~r["mask"]]
    assert np.array_equal(labels, rr["labels"])
    # fewer rounds, and a bar that nothing passes
    two = op.segment_planes(pts, pc.TAU, 2, pc.ROOM_MIN_INLIERS, pc.N_HYP, 0)
    assert two["n_planes"] == 2 and np.array_equal(two["planes"], rr["planes"][:2])
    assert np.array_equal(two["labels"], np.where(rr["labels"] < 2, rr["labels"], -1))
    assert op.segment_planes(pts, pc.TAU, 4, 2000, pc.N_HYP, 0)["n_planes"] == 0


def test_lattices_tie_of_count_and_sum_goes_to_the_smaller_hypothesis():
    r = op.segment_plane(pc.lattices(), 0.0, 64, 0)
    top = np.nonzero(r["counts"] == 25)[0]
    assert r["counts"].max() == 25 and top.shape[0] >= 2 and np.all(r["sums"][top] == 0.0)
    assert r["hypothesis"] == top[0] == 4
    assert r["inliers"].shape[0] == 25 and np.all(r["distance"][r["mask"]] == 0.0)
    assert np.array_equal(np.abs(r["plane"]), [0.0, 0.0, 1.0, float(r["point"][2])])


def test_a_point_exactly_at_the_threshold_is_inside():
    pts = pc.quarter_cloud()
    r = op.segment_plane(pts, 0.25, 64, 0, refine_iters=0)
    pl = r["build"]["planes"][r["hypothesis"]]
    assert np.array_equal(np.abs(pl[:3]), [0.0, 0.0, 1.0]) and pl[5] == 0.0
    assert r["count"] == 17 and r["mask"][16] and abs(r["distance"][16]) == 0.25
    below = op.segment_plane(pts, np.nextafter(0.25, 0.0), 64, 0, refine_iters=0)
    assert below["count"] == 16 and not below["mask"][16]


def test_collinear_cloud_has_no_valid_hypothesis():
    r = op.segment_plane(pc.collinear_cloud(), 0.1, 64, 0)
    assert r["n_valid"] == 0 and r["hypothesis"] == -1 and r["plane"] is None and r["point"] is None
    assert r["inliers"].shape == (0,) and not r["mask"].any()
    assert op.segment_planes(pc.collinear_cloud(), 0.1, 3)["n_planes"] == 0


def test_exact_translation_changes_no_decision():
    a, b = pc.grid_result(False), pc.grid_result(True)
    assert a["n_valid"] == 252 and a["hypothesis"] == 166
    for key in ("triples", "valid"):
        assert np.array_equal(a["build"][key], b["build"][key])
    assert np.array_equal(a["build"]["planes"][:, :3], b["build"]["planes"][:, :3])
    assert np.array_equal(a["build"]["planes"][:, 3:] + pc.SHIFT_EXACT * a["build"]["valid"][:, None], b["build"]["planes"][:, 3:])
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["sums"], b["sums"])
    assert a["hypothesis"] == b["hypothesis"]
    assert np.array_equal(a["mask"], b["mask"]) and a["inliers"].shape[0] == 202
    assert min(a["margin"], b["margin"]) > MARGIN


def test_draws_are_a_function_of_the_counter_alone():
    whole = op.draw(7, np.arange(0, 600, dtype=np.uint64), 2248)
    assert np.array_equal(op.draw(7, np.arange(300, 600, dtype=np.uint64), 2248), whole[300:])
    assert whole.min() >= 0 and whole.max() < 2248
    pts, _, _, _ = pc.table_scene()
    assert np.array_equal(op.build(pts, 7, 300, 300)["planes"], op.build(pts, 7, 600)["planes"][300:])
