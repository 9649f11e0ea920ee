"""Argument checks of the k-NN search and the outlier filters (probreg_amd.icp, probreg_amd.preprocess): every bad argument is a
ValueError before any GPU work, more than one rank a NotImplementedError."""
import numpy as np
import pytest

from probreg_amd import _lib, icp, preprocess
from probreg_amd import dist as pdist

CLOUD = np.random.default_rng(0).uniform(-1.0, 1.0, (40, 3))


@pytest.fixture(autouse=True)
def no_gpu_work(monkeypatch):
    def refuse():
        raise AssertionError("the GPU was asked for before the arguments were checked")

    monkeypatch.setattr(_lib, "require_gpu", refuse)


BAD_K = [0, 65, -1, 2.5, float("nan"), float("inf"), True, "8", None]
BAD_RADIUS = [0.0, -0.1, float("nan"), True, "0.1", None]


@pytest.mark.parametrize("k", BAD_K)
def test_bad_k(k):
    with pytest.raises(ValueError):
        icp.knn_search(CLOUD, CLOUD, k)
    with pytest.raises(ValueError):
        preprocess.remove_statistical_outlier(CLOUD, nb_neighbors=k)


@pytest.mark.parametrize("r", BAD_RADIUS)
def test_bad_radius(r):
    if r is not None:  # None is "no limit" for the search
        with pytest.raises(ValueError):
            icp.knn_search(CLOUD, CLOUD, 8, max_distance=r)
    with pytest.raises(ValueError):
        icp.radius_count(CLOUD, CLOUD, r)
    with pytest.raises(ValueError):
        preprocess.remove_radius_outlier(CLOUD, 5, r)


def test_an_infinite_radius_is_for_the_search_only():
    with pytest.raises(ValueError):
        icp.radius_count(CLOUD, CLOUD, float("inf"))
    with pytest.raises(ValueError):
        preprocess.remove_radius_outlier(CLOUD, 5, float("inf"))


@pytest.mark.parametrize("ratio", [-0.5, float("nan"), float("inf"), True, "2", None])
def test_bad_std_ratio(ratio):
    with pytest.raises(ValueError):
        preprocess.remove_statistical_outlier(CLOUD, 20, ratio)


@pytest.mark.parametrize("nb", [-1, 2.5, float("nan"), True, "5", None, 2 ** 31])
def test_bad_nb_points(nb):
    with pytest.raises(ValueError):
        preprocess.remove_radius_outlier(CLOUD, nb, 0.2)


def test_bad_clouds():
    bad = CLOUD.copy()
    bad[3, 1] = np.nan
    for cloud in (bad, CLOUD[:0], CLOUD[:, :1], np.zeros((4, 4)), CLOUD.reshape(2, 20, 3)):
        with pytest.raises(ValueError):
            preprocess.remove_statistical_outlier(cloud)
        with pytest.raises(ValueError):
            preprocess.remove_radius_outlier(cloud, 5, 0.2)
    for cloud in (bad, CLOUD[:0], CLOUD[:, :2]):
        with pytest.raises(ValueError):
            icp.knn_search(cloud, CLOUD, 4)
        with pytest.raises(ValueError):
            icp.knn_search(CLOUD, cloud, 4)
        with pytest.raises(ValueError):
            icp.radius_count(CLOUD, cloud, 0.2)


def test_bad_rows_that_ride_along():
    with pytest.raises(ValueError):
        preprocess.remove_statistical_outlier(CLOUD, normals=CLOUD[:-1])
    with pytest.raises(ValueError):
        preprocess.remove_statistical_outlier(CLOUD[:, :2], normals=CLOUD)  # normals of a 2-D cloud have two columns
    with pytest.raises(ValueError):
        preprocess.remove_radius_outlier(CLOUD, 5, 0.2, attributes=np.zeros(40))
    nan = np.zeros((40, 2))
    nan[0, 0] = np.inf
    with pytest.raises(ValueError):
        preprocess.remove_radius_outlier(CLOUD, 5, 0.2, attributes=nan)


def test_more_than_one_rank_is_refused(monkeypatch):
    monkeypatch.setattr(pdist, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        preprocess.remove_statistical_outlier(CLOUD)
    with pytest.raises(NotImplementedError):
        preprocess.remove_radius_outlier(CLOUD, 5, 0.2)
    with pytest.raises(NotImplementedError):
        icp.knn_search(CLOUD, CLOUD, 4)
    with pytest.raises(NotImplementedError):
        icp.radius_count(CLOUD, CLOUD, 0.2)


def test_plan_methods_check_before_the_library_is_called():
    plan = icp.IcpPlan.__new__(icp.IcpPlan)  # no handle: a call into the library would fail on it
    plan._h = None
    for k in BAD_K:
        with pytest.raises(ValueError):
            plan.knn(k)
    for r in BAD_RADIUS:
        if r is not None:
            with pytest.raises(ValueError):
                plan.knn(4, r)
        with pytest.raises(ValueError):
            plan.radius_count(r)
    import ctypes

    most = ctypes.c_int(0)
    _lib.check(_lib.lib.prg_icp_max_k(ctypes.byref(most)))
    assert icp.MAX_K == most.value == 64
    assert _lib.lib.prg_icp_max_k(None) == _lib.PRG_ERR_INVALID
