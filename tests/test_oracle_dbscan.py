"""The DBSCAN restatement (tests/oracle_dbscan.py) on the host: the figures of the scene that the GPU
tests use, so that it cannot drift; the recovery of its three objects; scikit-learn's DBSCAN where it is installed, in
everything the definitions share (core set, labels of the core points, noise set, border points that touch one cluster);
and the tie rule of the border points.  No GPU."""
import numpy as np
import pytest

import dbscan_cases as dc
import oracle_dbscan as od
from probreg_amd import synthetic

# (eps, min_points): clusters, sizes, core, border, noise, ambiguous border points, least |d2 - eps eps| / (eps eps) to two digits
FIGURES = {
    (0.25, 8): (3, [902, 602, 303], 1804, 3, 73, 0, 1.2e-5),
    (0.15, 10): (6, [597, 186, 858, 75, 27, 10], 1474, 279, 127, 4, 4.4e-5),
}


@pytest.mark.parametrize("params", dc.PARAMS)
def test_scene_figures(params):
    cloud, _ = dc.scene(synthetic)
    ref = dc.scene_ref(synthetic, *params)
    n_clusters, sizes, core, border, noise, ambiguous, gap = FIGURES[params]
    labels = ref["labels"]
    print("eps %g min_points %d: %d clusters %s, core %d, border %d, noise %d, ambiguous %d, gap %.3g"
          % (params + (ref["n_clusters"], ref["sizes"].tolist(), int(ref["core"].sum()),
                       int(np.sum(~ref["core"] & (labels >= 0))), int(np.sum(labels < 0)), ref["ambiguous"].shape[0], ref["gap"])))
    assert cloud.shape == (1880, 3)
    assert ref["n_clusters"] == n_clusters and ref["sizes"].tolist() == sizes
    assert int(ref["core"].sum()) == core
    assert int(np.sum(~ref["core"] & (labels >= 0))) == border
    assert int(np.sum(labels < 0)) == noise
    assert ref["ambiguous"].shape[0] == ambiguous
    assert float("%.1e" % ref["gap"]) == gap
    assert labels.dtype == np.int32 and ref["counts"].dtype == np.int32 and ref["sizes"].dtype == np.int32
    assert int(ref["sizes"].sum()) == int(np.sum(labels >= 0))
    # the numbering: cluster c starts at its smallest core index, ascending in c
    firsts = [int(np.nonzero(ref["core"] & (labels == c))[0][0]) for c in range(n_clusters)]
    assert firsts == sorted(firsts)


def test_scene_objects_are_recovered():
    """At (0.25, 8) every object is one cluster, no object point is noise, and 7 outliers are absorbed."""
    _, origin = dc.scene(synthetic)
    labels = dc.scene_ref(synthetic, 0.25, 8)["labels"]
    obj = origin >= 0
    assert np.all(labels[obj] >= 0)
    names = [np.unique(labels[origin == o]) for o in range(3)]
    assert all(u.shape[0] == 1 for u in names) and sorted(int(u[0]) for u in names) == [0, 1, 2]
    for o in range(3):  # object membership equals cluster membership among the object points
        assert np.array_equal(labels[obj] == names[o][0], origin[obj] == o)
    assert int(np.sum(labels[~obj] >= 0)) == 7


@pytest.mark.parametrize("params", dc.PARAMS)
def test_scene_against_scikit_learn(params):
    cluster = pytest.importorskip("sklearn.cluster")
    cloud, _ = dc.scene(synthetic)
    ref = dc.scene_ref(synthetic, *params)
    sk = cluster.DBSCAN(eps=params[0], min_samples=params[1], algorithm="brute").fit(cloud)
    core = np.zeros(cloud.shape[0], dtype=bool)
    core[sk.core_sample_indices_] = True
    assert np.array_equal(core, ref["core"])
    assert np.array_equal(sk.labels_[core], ref["labels"][core])
    assert np.array_equal(sk.labels_ < 0, ref["labels"] < 0)
    single = ~core & (ref["labels"] >= 0)
    single[ref["ambiguous"]] = False
    assert np.array_equal(sk.labels_[single], ref["labels"][single])


@pytest.mark.parametrize("left_first", [False, True])
def test_tie_goes_to_the_smaller_core_index(left_first):
    cloud, eps, min_points = dc.tie_cloud(left_first)
    ref = od.dbscan(cloud, eps, min_points)
    assert ref["gap"] == 0.0  # d2 == eps eps occurs: the ball is closed
    assert ref["counts"].tolist() == [5, 4, 4, 4, 5, 4, 4, 4, 3]
    assert ref["core"].tolist() == [True] * 8 + [False]
    assert ref["labels"].tolist() == [0] * 4 + [1] * 4 + [0]
    assert ref["ambiguous"].tolist() == [8] and ref["sizes"].tolist() == [5, 4]
    assert (cloud[0, 0] < 0.0) == left_first


def test_noise_single_points_and_min_points_one():
    one = np.array([[1.0, 2.0, 3.0]])
    assert od.dbscan(one, 0.5, 1)["labels"].tolist() == [0]
    ref = od.dbscan(one, 0.5, 2)
    assert ref["labels"].tolist() == [-1] and ref["n_clusters"] == 0 and ref["sizes"].shape == (0,)
    cloud, _ = dc.scene(synthetic)
    ref = dc.scene_ref(synthetic, 0.15, 1)
    assert np.all(ref["core"]) and np.all(ref["labels"] >= 0) and int(ref["sizes"].sum()) == cloud.shape[0]
    assert [c.tolist() for c in od.clusters(od.dbscan(dc.tie_cloud()[0], 1.0, 4), 5)] == [[0, 1, 2, 3, 8]]
