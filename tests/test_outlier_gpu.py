"""The outlier filters on the GPU (preprocess.remove_statistical_outlier / remove_radius_outlier, csrc/icp_outlier.hip) against their
restatement (tests/oracle_knn.py) on the target of filterreg_pair(2000), which has 100 uniform outliers.

Masks and kept indices must equal the restatement's: tests/test_oracle_knn.py shows that no decision of these cases lies
within 1e-9 (relative) of its threshold, so no point is excused.  The radius score is an integer and exact.  The statistical
score adds the same k square roots in the same order as the restatement, one rounding per square root and per addition and
one for the division: (k + 2) 2^-52 relative.  thr is held to 1e-9 relative, which the gap rule needs.
"""
import numpy as np
import pytest

import oracle_knn as ok
from probreg_amd import synthetic

pytestmark = pytest.mark.gpu

K = 20


def _pre():
    from probreg_amd import preprocess
    return preprocess


@pytest.mark.parametrize("std_ratio", [2.0, 1.0])
def test_statistical_filter_equals_the_restatement(std_ratio):
    cloud = ok.filter_cloud(synthetic)
    ref = ok.cached(("statistical", K, std_ratio), lambda: ok.statistical(cloud, K, std_ratio))
    got = _pre().remove_statistical_outlier(cloud, K, std_ratio)
    mu, s, thr = got.threshold
    score_err = float(np.max(np.abs(got.score - ref["score"]) / ref["score"]))
    thr_err = abs(thr - ref["thr"]) / ref["thr"]
    print("std_ratio %g: kept %d of %d, score differs by %.3g relative (bound %.3g), mu %.3g, s %.3g, thr %.3g relative"
          % (std_ratio, got.index.shape[0], cloud.shape[0], score_err, (K + 2) * 2.0 ** -52, abs(mu - ref["mu"]) / ref["mu"],
             abs(s - ref["s"]) / ref["s"], thr_err))
    assert got.mask.dtype == np.bool_ and got.index.dtype == np.int32
    assert np.array_equal(got.mask, ref["mask"]) and np.array_equal(got.index, ref["index"])
    assert np.array_equal(got.points, cloud[ref["index"]])
    assert score_err <= (K + 2) * 2.0 ** -52
    assert thr_err <= 1.0e-9 and abs(mu - ref["mu"]) <= 1.0e-9 * ref["mu"] and abs(s - ref["s"]) <= 1.0e-9 * ref["s"]
    assert got.normals is None and got.attributes is None


def test_radius_filter_equals_the_restatement():
    cloud = ok.filter_cloud(synthetic)
    ref = ok.cached(("radius", 10, 0.15), lambda: ok.radius(cloud, 10, 0.15))
    got = _pre().remove_radius_outlier(cloud, 10, 0.15)
    assert got.score.dtype == np.int32 and got.score.tobytes() == ref["score"].astype(np.int32).tobytes()
    assert np.array_equal(got.mask, ref["mask"]) and np.array_equal(got.index, ref["index"])
    assert np.array_equal(got.points, cloud[ref["index"]]) and got.threshold == 10
    assert 0 < got.index.shape[0] < cloud.shape[0]


def test_a_cloud_of_equal_scores_is_kept():
    """Eight corners of a cube, k = 4: every a_i = (0 + 2 + 2 + 2) / 4, s = 0, thr = mu = a_i.  A strict < would drop all."""
    cube = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    got = _pre().remove_statistical_outlier(cube, 4, 2.0)
    assert np.all(got.score == 1.5) and got.threshold == (1.5, 0.0, 1.5)
    assert np.all(got.mask) and got.index.tolist() == list(range(8)) and np.array_equal(got.points, cube)


def test_coincident_copies_are_kept():
    """Eight copies of a cloud, k = 8: every a_i = 0 (Open3D drops a point with a_i = 0)."""
    cloud = np.ascontiguousarray(np.tile(synthetic.surface(300, 1), (8, 1)))
    got = _pre().remove_statistical_outlier(cloud, 8, 2.0)
    assert np.all(got.score == 0.0) and got.threshold == (0.0, 0.0, 0.0) and np.all(got.mask)
    assert got.index.shape[0] == cloud.shape[0]


def test_a_single_point():
    got = _pre().remove_statistical_outlier(np.array([[1.0, 2.0, 3.0]]), 20, 2.0)
    assert got.mask.tolist() == [True] and got.threshold == (0.0, 0.0, 0.0)
    got = _pre().remove_radius_outlier(np.array([[1.0, 2.0, 3.0]]), 0, 0.5)
    assert got.mask.tolist() == [True] and got.score.tolist() == [1]
    got = _pre().remove_radius_outlier(np.array([[1.0, 2.0, 3.0]]), 1, 0.5)
    assert got.mask.tolist() == [False] and got.points.shape == (0, 3)


def test_normals_and_attributes_follow_the_index():
    cloud = ok.filter_cloud(synthetic)
    rng = np.random.default_rng(2)
    normals, attributes = rng.normal(size=cloud.shape), rng.uniform(size=(cloud.shape[0], 5))
    ref = ok.cached(("statistical", K, 2.0), lambda: ok.statistical(cloud, K, 2.0))
    got = _pre().remove_statistical_outlier(cloud, K, 2.0, normals=normals, attributes=attributes)
    assert np.array_equal(got.index, ref["index"])
    assert np.array_equal(got.normals, normals[got.index]) and np.array_equal(got.attributes, attributes[got.index])

    class Cloud(object):
        pass

    obj = Cloud()
    obj.points, obj.normals = cloud, normals
    got = _pre().remove_radius_outlier(obj, 10, 0.15)
    ref = ok.cached(("radius", 10, 0.15), lambda: ok.radius(cloud, 10, 0.15))
    assert np.array_equal(got.index, ref["index"]) and np.array_equal(got.normals, normals[ref["index"]])


def test_a_2d_cloud_is_its_padding_with_zeros():
    flat = np.ascontiguousarray(ok.filter_cloud(synthetic)[:, :2])
    padded = np.ascontiguousarray(np.concatenate([flat, np.zeros((flat.shape[0], 1))], axis=1))
    a, b = _pre().remove_statistical_outlier(flat, K, 1.0), _pre().remove_statistical_outlier(padded, K, 1.0)
    assert a.points.shape[1] == 2 and np.array_equal(a.points, b.points[:, :2])
    assert np.array_equal(a.index, b.index) and a.score.tobytes() == b.score.tobytes() and a.threshold == b.threshold
    assert 0 < a.index.shape[0] < flat.shape[0]
    a, b = _pre().remove_radius_outlier(flat, 10, 0.1), _pre().remove_radius_outlier(padded, 10, 0.1)
    assert np.array_equal(a.index, b.index) and a.score.tobytes() == b.score.tobytes()
    ref = ok.radius(padded, 10, 0.1)
    assert np.array_equal(a.index, ref["index"])
