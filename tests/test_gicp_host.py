"""Generalized ICP of probreg_amd.icp on the host: input validation before anything reaches the device, the host mirror of the
covariances against the restatement, and that the existing estimators' names are as they were."""
import numpy as np
import pytest

import oracle_gicp as ogi
from probreg_amd import _lib, icp, synthetic


def _pair():
    src, tgt, tn, _ = synthetic.pt2pl_pair(60, m=50, seed=1)
    sn = synthetic.surface_with_normals(50, 1)[1]
    return src, tgt, sn, tn


def _spd(n, seed=0):
    a = np.random.default_rng(seed).normal(size=(n, 3, 3))
    return a @ a.transpose(0, 2, 1) + 0.1 * np.eye(3)


def test_validation_errors():
    src, tgt, sn, tn = _pair()
    ok = dict(source_normals=sn, target_normals=tn)
    nan = sn.copy()
    nan[3, 1] = np.nan
    zero = tn.copy()
    zero[7] = 0.0
    cs, ct = _spd(50), _spd(60, 1)
    skew = cs.copy()
    skew[4, 0, 1] += 1.0e-9
    flat = cs.copy()
    flat[5] = np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])  # rank 1: a pivot at the floor
    negative = ct.copy()
    negative[2] = -np.eye(3)
    inf = ct.copy()
    inf[0, 2, 2] = np.inf
    for call in (
        lambda: icp.registration_gicp(src[:, :2], tgt, 0.1, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.0, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, init=np.eye(3), **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, max_iteration=-1, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, relative_fitness=np.nan, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, epsilon=0.0, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, epsilon=1.5, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, epsilon=-1.0e-3, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, epsilon=np.nan, **ok),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_normals=sn[:-1], target_normals=tn),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_normals=sn, target_normals=tn[:, :2]),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_normals=nan, target_normals=tn),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_normals=sn, target_normals=zero),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_covariances=cs[:-1], target_covariances=ct),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_covariances=cs.reshape(50, 9), target_covariances=ct),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_covariances=skew, target_covariances=ct),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_covariances=flat, target_covariances=ct),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_covariances=cs, target_covariances=negative),
        lambda: icp.registration_gicp(src, tgt, 0.1, source_covariances=cs, target_covariances=inf),
        lambda: icp.registration_gicp(src, tgt, 0.1, normal_radius=-0.1),
        lambda: icp.covariances_from_normals(zero),
        lambda: icp.covariances_from_normals(nan),
        lambda: icp.covariances_from_normals(sn, epsilon=0.0),
        lambda: icp.covariances_from_normals(sn.reshape(-1)),
    ):
        with pytest.raises(ValueError):
            call()


def test_messages_name_the_fault():
    src, tgt, sn, tn = _pair()
    zero = tn.copy()
    zero[7] = 0.0
    with pytest.raises(ValueError, match="target_normals: row 7 has norm 0"):
        icp.registration_gicp(src, tgt, 0.1, source_normals=sn, target_normals=zero)
    with pytest.raises(ValueError, match="epsilon"):
        icp.registration_gicp(src, tgt, 0.1, source_normals=sn, target_normals=tn, epsilon=2.0)
    flat = _spd(50)
    flat[5] = np.outer([1.0, 2.0, 3.0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="source_covariances: covariance 5 is not positive definite"):
        icp.registration_gicp(src, tgt, 0.1, source_covariances=flat, target_normals=tn)
    skew = _spd(60)
    skew[4, 0, 1] += 1.0e-9
    with pytest.raises(ValueError, match="target_covariances must be symmetric"):
        icp.registration_gicp(src, tgt, 0.1, source_normals=sn, target_covariances=skew)


def test_without_normals_the_message_points_to_the_normal_estimation():
    src, tgt, sn, tn = _pair()
    with pytest.raises(ValueError, match="estimate_normals"):
        icp.registration_gicp(src, tgt, 0.1)
    with pytest.raises(ValueError, match="of the target.*estimate_normals"):
        icp.registration_gicp(src, tgt, 0.1, source_normals=sn)

    class Cloud(object):
        points, normals = tgt, np.zeros((0, 3))  # an empty .normals is none

    with pytest.raises(ValueError, match="estimate_normals"):
        icp.registration_gicp(src, Cloud(), 0.1, source_normals=sn)


def test_host_mirror_equals_the_restatement():
    _, _, sn, tn = _pair()
    for nrm, eps in ((sn, 1.0e-3), (-2.5 * tn, 0.05), (tn.astype(np.float32).astype(np.float64), 1.0)):
        got = icp.covariances_from_normals(nrm, eps)
        assert got.shape == (nrm.shape[0], 3, 3) and got.tobytes() == ogi.full(ogi.covariances_from_normals(nrm, eps)).tobytes()
        assert np.array_equal(got, got.transpose(0, 2, 1))
        assert icp._checked_cov6(got, "covariances").tobytes() == ogi.covariances_from_normals(nrm, eps).tobytes()


def test_existing_names_are_as_they_were():
    assert (icp.POINT_TO_POINT, icp.POINT_TO_PLANE, icp.GENERALIZED, icp.N_SUMS) == (0, 1, 2, 32)
    assert icp.IcpResult._fields == ("transformation", "fitness", "inlier_rmse", "correspondences", "n_iter", "converged")
    assert icp.GicpResult._fields == icp.IcpResult._fields + ("objective",)
    assert icp._plan_kind(2) == icp._plan_kind("generalized") == 2 and icp._plan_kind("point_to_plane") == 1
    for bad in (2, "generalized", 3):
        with pytest.raises(ValueError):
            icp._kind(bad)  # registration_icp does not take the generalized estimator: registration_gicp does
    with pytest.raises(ValueError):
        icp._plan_kind(3)


def test_more_than_one_rank_is_refused(monkeypatch):
    from probreg_amd import dist as pdist

    src, tgt, sn, tn = _pair()
    monkeypatch.setattr(pdist, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        icp.registration_gicp(src, tgt, 0.1, source_normals=sn, target_normals=tn)


def test_valid_input_reaches_the_library():
    """Without a GPU every entry raises ProbregHipError once validation has passed (no CPU fallback); with one it runs."""
    src, tgt, sn, tn = _pair()

    class Cloud(object):
        def __init__(self, points, normals):
            self.points, self.normals = points, normals

    calls = (lambda: icp.registration_gicp(src, tgt, 0.5, source_normals=sn, target_normals=tn),
             lambda: icp.registration_gicp(Cloud(src, sn), Cloud(tgt, tn), np.inf, init=np.eye(4)),
             lambda: icp.registration_gicp(src, tgt, 0.5, source_covariances=_spd(50), target_covariances=_spd(60, 1)[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]),
             lambda: icp.registration_gicp(src, tgt, 0.5, normal_radius=0.5))
    for call in calls:
        if _lib.device_count() > 0:
            assert call() is not None
        else:
            with pytest.raises(_lib.ProbregHipError):
                call()
