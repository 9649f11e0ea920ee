"""The yardstick of the k-NN and outlier-filter GPU tests (tests/oracle_knn.py), pinned on the host: its
lists against scipy's kd-tree, and the decision gaps that let the GPU tests demand equal masks with no point excused."""
import numpy as np
import pytest
from scipy import spatial  # the yardstick's own yardstick: a missing scipy fails, it does not skip

import oracle_knn as ok
from probreg_amd import synthetic


def test_lists_equal_the_kd_tree_where_its_distances_differ():
    q = synthetic.surface(300, 5)
    y = synthetic.surface(1500, 6)
    for k in (1, 8, 20):
        idx, d2, cnt = ok.knn(q, y, k)
        dist, tree_idx = spatial.cKDTree(y).query(q, k=k)
        dist, tree_idx = dist.reshape(q.shape[0], k), tree_idx.reshape(q.shape[0], k)
        assert np.all(cnt == k) and idx.dtype == np.int32
        assert np.allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0.0)
        # a slot is decided when its distance differs from both neighbours' in the tree's own list
        lone = np.ones_like(dist, dtype=bool)
        lone[:, 1:] &= dist[:, 1:] != dist[:, :-1]
        lone[:, :-1] &= dist[:, :-1] != dist[:, 1:]
        assert lone.mean() > 0.99
        assert np.array_equal(idx[lone], tree_idx[lone])


def test_lists_radius_ties_and_padding():
    y = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 3.0, 4.0]])
    idx, d2, cnt = ok.knn(y[:1], y, 3)
    assert idx.tolist() == [[0, 2, 1]] and d2.tolist() == [[0.0, 0.0, 1.0]] and cnt.tolist() == [3]
    idx, d2, cnt = ok.knn(y[:1], y, 4, r=5.0)  # equality counts as inside
    assert idx.tolist() == [[0, 2, 1, 3]] and d2[0, 3] == 25.0 and cnt.tolist() == [4]
    idx, d2, cnt = ok.knn(y[:1], y, 4, r=np.nextafter(5.0, 0.0))
    assert idx.tolist() == [[0, 2, 1, -1]] and np.isposinf(d2[0, 3]) and cnt.tolist() == [3]
    assert ok.radius_count(y[:1], y, 5.0).tolist() == [4] and ok.radius_count(y[:1], y, 4.9).tolist() == [3]
    idx, d2, cnt = ok.knn(y, y[:1], 64)
    assert cnt.tolist() == [1, 1, 1, 1] and np.all(idx[:, 1:] == -1) and np.all(np.isposinf(d2[:, 1:]))


def test_run_sum_order():
    v = np.random.default_rng(0).uniform(0.0, 1.0, 200)
    part = [0.0, 0.0, 0.0, 0.0]
    for r in range(4):
        for x in v[64 * r:64 * r + 64]:
            part[r] = part[r] + x
    assert ok.run_sum(v) == ((part[0] + part[1]) + part[2]) + part[3]


@pytest.mark.parametrize("std_ratio, removed, gap", [(2.0, 70, 1.9e-3), (1.0, 84, 2.0e-2)])
def test_statistical_filter_gaps(std_ratio, removed, gap):
    """The GPU test demands the restatement's mask: no a_i may lie within GAP of the threshold."""
    cloud = ok.filter_cloud(synthetic)
    assert cloud.shape == (2000, 3)
    res = ok.cached(("statistical", 20, std_ratio), lambda: ok.statistical(cloud, 20, std_ratio))
    print("std_ratio %g: removed %d, mu %.6g, s %.6g, thr %.6g, least gap %.3g"
          % (std_ratio, 2000 - res["index"].shape[0], res["mu"], res["s"], res["thr"], res["gap"]))
    assert 2000 - res["index"].shape[0] == removed
    assert 0.9 * gap <= res["gap"] <= 1.1 * gap
    assert int(np.sum(np.abs(res["score"] - res["thr"]) <= ok.GAP * res["thr"])) == 0  # excused points: none


def test_radius_filter_gap():
    cloud = ok.filter_cloud(synthetic)
    res = ok.cached(("radius", 10, 0.15), lambda: ok.radius(cloud, 10, 0.15))
    print("radius 0.15, nb_points 10: removed %d, least gap %.3g" % (2000 - res["index"].shape[0], res["gap"]))
    assert 2000 - res["index"].shape[0] == 119
    assert 0.9 * 2.8e-5 <= res["gap"] <= 1.1 * 2.8e-5 and res["gap"] > ok.GAP


def test_degenerate_clouds_are_kept():
    cube = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    res = ok.statistical(cube, 4, 2.0)  # itself at 0 and three neighbours at 2
    assert np.all(res["score"] == 1.5) and res["s"] == 0.0 and res["thr"] == 1.5 and np.all(res["mask"])
    copies = np.tile(synthetic.surface(50, 1), (8, 1))
    res = ok.statistical(copies, 8, 2.0)
    assert np.all(res["score"] == 0.0) and np.all(res["mask"])
    one = ok.statistical(np.zeros((1, 3)), 20, 2.0)
    assert one["s"] == 0.0 and one["mask"].tolist() == [True]
