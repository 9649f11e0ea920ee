"""DBSCAN on the GPU (preprocess.cluster_dbscan, csrc/icp_cluster.hip) against its restatement (tests/oracle_dbscan.py, DESIGN.md
section 3.19).

labels, core, counts, n_clusters and sizes must equal the restatement's byte for byte: both sides decide d2 <= eps eps on the
same bits, d2 = (dx dx + dy dy) + dz dz in fp64 without contraction, and the numbering is canonical, so no point is excused
whatever the margin of a case is (tests/test_oracle_dbscan.py pins the scene's figures).  The clouds are in
tests/dbscan_cases.py.
"""
import numpy as np
import pytest

import dbscan_cases as dc
import oracle_dbscan as od
import oracle_knn as ok
from probreg_amd import synthetic

pytestmark = pytest.mark.gpu


def _pre():
    from probreg_amd import preprocess
    return preprocess


def _equal(got, ref):
    assert got.labels.dtype == np.int32 and got.core.dtype == np.bool_ and got.counts.dtype == np.int32
    assert got.sizes.dtype == np.int32 and isinstance(got.n_clusters, int)
    assert got.counts.tobytes() == ref["counts"].tobytes()
    assert got.core.tobytes() == ref["core"].tobytes()
    assert got.n_clusters == ref["n_clusters"]
    assert got.labels.tobytes() == ref["labels"].tobytes()
    assert got.sizes.shape == (ref["n_clusters"],) and got.sizes.tobytes() == ref["sizes"].tobytes()


@pytest.mark.parametrize("params", dc.PARAMS + ((0.15, 1),))
def test_scene_equals_the_restatement(params):
    cloud, _ = dc.scene(synthetic)
    ref = dc.scene_ref(synthetic, *params)
    got = _pre().cluster_dbscan(cloud, *params)
    print("eps %g min_points %d: %d clusters %s, %d core, %d noise" % (params + (got.n_clusters, got.sizes.tolist(),
                                                                               int(got.core.sum()), int(np.sum(got.labels < 0)))))
    _equal(got, ref)
    if params[1] == 1:  # every point is core: the components of the eps graph, no border, no noise
        assert np.all(got.core) and np.all(got.labels >= 0) and int(got.sizes.sum()) == cloud.shape[0]


def test_the_grid_does_not_show():
    """One cell, the cloud's own edge, a fine dense grid and a hashed one: the same labels."""
    from probreg_amd import icp

    cloud, _ = dc.scene(synthetic)
    ref = dc.scene_ref(synthetic, 0.15, 10)
    seen = []
    for edge in (None, 0.01, 0.3, 8.0):
        plan = icp.IcpPlan()
        try:
            plan.set_target(cloud, cell_edge=edge)
            plan.set_source(cloud)
            labels, core, counts, n_clusters, sizes = plan._dbscan(0.15, 10)
            seen.append((plan.grid()[1:3], labels.tobytes()))
        finally:
            plan.close()
        print("cell_edge %r: grid %s, dense %s" % (edge, list(seen[-1][0][0]), seen[-1][0][1]))
        assert labels.tobytes() == ref["labels"].tobytes() and core.tobytes() == ref["core"].tobytes()
        assert counts.tobytes() == ref["counts"].tobytes() and n_clusters == ref["n_clusters"]
        assert sizes.tobytes() == ref["sizes"].tobytes()
    assert any(not dense for (_, dense), _ in seen) and any(max(dims) == 1 for (dims, _), _ in seen)


def test_the_same_call_twice_gives_equal_bytes():
    cloud, _ = dc.scene(synthetic)
    a, b = _pre().cluster_dbscan(cloud, 0.15, 10), _pre().cluster_dbscan(cloud, 0.15, 10)
    for x, y in zip(a, b):
        assert (x == y) if isinstance(x, int) else (x.tobytes() == y.tobytes())


@pytest.mark.parametrize("min_points,core,border", [(2, 3000, 0), (3, 2998, 2)])
def test_a_chain_of_3000_points_is_one_cluster(min_points, core, border):
    """The deepest tree the union-find sees: every link joins two neighbours of a path in a random order."""
    cloud = dc.chain()
    ref = od.cached(("dbscan_chain", min_points), lambda: od.dbscan(cloud, 0.1, min_points))
    got = _pre().cluster_dbscan(cloud, 0.1, min_points)
    _equal(got, ref)
    assert got.n_clusters == 1 and got.sizes.tolist() == [3000] and int(got.core.sum()) == core
    assert int(np.sum(~got.core & (got.labels == 0))) == border and not np.any(got.labels < 0)


def test_coincident_copies_are_all_core():
    cloud = np.ascontiguousarray(np.tile(synthetic.surface(300, 1), (8, 1)))
    ref = od.cached("dbscan_copies", lambda: od.dbscan(cloud, 0.1, 8))
    got = _pre().cluster_dbscan(cloud, 0.1, 8)
    _equal(got, ref)
    assert np.all(got.core) and np.all(got.counts >= 8) and np.array_equal(got.labels[:300], got.labels[2100:])


@pytest.mark.parametrize("left_first", [False, True])
def test_a_tie_goes_to_the_smaller_core_index(left_first):
    cloud, eps, min_points = dc.tie_cloud(left_first)
    got = _pre().cluster_dbscan(cloud, eps, min_points)
    _equal(got, od.dbscan(cloud, eps, min_points))
    assert got.labels.tolist() == [0] * 4 + [1] * 4 + [0] and got.core.tolist() == [True] * 8 + [False]


def test_the_ball_is_closed():
    """eps = 5/16 and points exactly 5/16 apart ((3/16, 4/16, 0): d2 = 25/256 exactly): d2 == eps eps is inside."""
    cloud = np.array([[0.0, 0.0, 0.0], [0.1875, 0.25, 0.0], [0.375, 0.5, 0.0], [0.375, 0.5, 0.3125], [2.0, 2.0, 2.0]])
    got = _pre().cluster_dbscan(cloud, 0.3125, 2)
    _equal(got, od.dbscan(cloud, 0.3125, 2))
    assert got.counts.tolist() == [2, 3, 3, 2, 1] and got.labels.tolist() == [0, 0, 0, 0, -1] and got.sizes.tolist() == [4]
    got = _pre().cluster_dbscan(cloud, 0.3125, 3)
    _equal(got, od.dbscan(cloud, 0.3125, 3))
    assert got.core.tolist() == [False, True, True, False, False] and got.labels.tolist() == [0, 0, 0, 0, -1]


def test_a_single_point():
    one = np.array([[1.0, 2.0, 3.0]])
    got = _pre().cluster_dbscan(one, 0.5, 1)
    assert got.labels.tolist() == [0] and got.core.tolist() == [True] and got.counts.tolist() == [1]
    assert got.n_clusters == 1 and got.sizes.tolist() == [1]
    got = _pre().cluster_dbscan(one, 0.5, 2)
    assert got.labels.tolist() == [-1] and got.core.tolist() == [False] and got.n_clusters == 0 and got.sizes.shape == (0,)


def test_min_points_above_n_is_all_noise():
    cloud = synthetic.surface(200, 3)
    got = _pre().cluster_dbscan(cloud, 0.2, 201)
    assert np.all(got.labels == -1) and not np.any(got.core) and got.n_clusters == 0
    assert got.sizes.shape == (0,) and got.sizes.dtype == np.int32 and got.clusters() == []


def test_a_far_point_does_not_change_the_scene():
    cloud, _ = dc.scene(synthetic)
    far = np.ascontiguousarray(np.concatenate([cloud, np.full((1, 3), 1.0e6)], axis=0))
    ref = od.cached(("dbscan_far", 0.15, 10), lambda: od.dbscan(far, 0.15, 10))
    got = _pre().cluster_dbscan(far, 0.15, 10)
    _equal(got, ref)
    assert got.labels[-1] == -1 and got.counts[-1] == 1
    assert got.labels[:-1].tobytes() == dc.scene_ref(synthetic, 0.15, 10)["labels"].tobytes()


def test_a_2d_cloud_is_its_padding_with_zeros():
    flat = np.ascontiguousarray(dc.scene(synthetic)[0][:, :2])
    padded = np.ascontiguousarray(np.concatenate([flat, np.zeros((flat.shape[0], 1))], axis=1))
    a, b = _pre().cluster_dbscan(flat, 0.1, 10), _pre().cluster_dbscan(padded, 0.1, 10)
    _equal(a, od.cached(("dbscan_flat", 0.1, 10), lambda: od.dbscan(padded, 0.1, 10)))
    for x, y in zip(a, b):
        assert (x == y) if isinstance(x, int) else (x.tobytes() == y.tobytes())
    assert a.n_clusters >= 1 and np.any(a.labels < 0)


def test_clusters_hands_over_the_index_arrays():
    cloud, _ = dc.scene(synthetic)
    ref = dc.scene_ref(synthetic, 0.15, 10)
    got = _pre().cluster_dbscan(cloud, 0.15, 10)
    mine, theirs = got.clusters(min_size=50), od.clusters(ref, 50)
    assert len(mine) == len(theirs) == 4
    for a, b in zip(mine, theirs):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert [c.shape[0] for c in got.clusters()] == got.sizes.tolist()

    class Cloud(object):
        pass

    obj = Cloud()
    obj.points = cloud
    assert _pre().cluster_dbscan(obj, 0.15, 10).labels.tobytes() == got.labels.tobytes()


def test_argument_errors_come_before_the_device(monkeypatch):
    from probreg_amd import icp

    def no_plan(*a, **k):
        raise AssertionError("a plan was created")

    monkeypatch.setattr(icp, "IcpPlan", no_plan)
    cloud = synthetic.surface(50, 0)
    for eps in (0.0, -0.1, float("nan"), float("inf"), True, "0.1", None):
        with pytest.raises(ValueError):
            _pre().cluster_dbscan(cloud, eps, 5)
    for min_points in (0, -3, 2.5, 2 ** 31, float("nan"), float("inf"), True, "5", None):
        with pytest.raises(ValueError):
            _pre().cluster_dbscan(cloud, 0.1, min_points)
    for points in (np.zeros((5, 4)), np.zeros((0, 3)), np.full((5, 3), np.nan)):
        with pytest.raises(ValueError):
            _pre().cluster_dbscan(points, 0.1, 5)


def test_the_plan_refuses_what_the_kernels_cannot_index():
    from probreg_amd import _lib, icp

    cloud = synthetic.surface(60, 0)
    plan = icp.IcpPlan()
    try:
        plan.set_target(cloud)
        plan.set_source(cloud[:50])
        with pytest.raises(_lib.ProbregHipError):  # 60 target points, 50 source points
            plan._dbscan(0.1, 5)
        plan.set_source(cloud)
        with pytest.raises(ValueError):
            plan._dbscan(0.1, 0)
        with pytest.raises(ValueError):
            plan._dbscan(float("inf"), 5)
        with pytest.raises(_lib.ProbregHipError):  # nothing to read yet
            _lib.check(_lib.lib.prg_icp_get_dbscan(plan._h, None, None, None, None))
    finally:
        plan.close()


def test_the_radius_filter_is_unchanged_afterwards():
    """The radius count shares its walk with the link kernel: after a clustering, on a fresh plan, it still equals its restatement."""
    cloud = ok.filter_cloud(synthetic)
    _pre().cluster_dbscan(cloud, 0.15, 10)
    ref = ok.cached(("radius", 10, 0.15), lambda: ok.radius(cloud, 10, 0.15))
    got = _pre().remove_radius_outlier(cloud, 10, 0.15)
    assert got.score.tobytes() == ref["score"].astype(np.int32).tobytes()
    assert np.array_equal(got.mask, ref["mask"]) and np.array_equal(got.index, ref["index"])
