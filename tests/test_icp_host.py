"""probreg_amd.icp on the host: input validation, and that nothing is computed without a GPU."""
import numpy as np
import pytest

from probreg_amd import _lib, icp, synthetic
from probreg_amd.transformation import RigidTransformation


def _pair():
    src, tgt, nrm, _ = synthetic.pt2pl_pair(60, m=50, seed=1)
    return src, tgt, nrm


def test_validation_errors():
    src, tgt, nrm = _pair()
    bad = src.copy()
    bad[3, 1] = np.nan
    for call in (
        lambda: icp.registration_icp(src[:, :2], tgt, 0.1),
        lambda: icp.registration_icp(src, tgt.reshape(-1), 0.1),
        lambda: icp.registration_icp(np.zeros((0, 3)), tgt, 0.1),
        lambda: icp.registration_icp(bad, tgt, 0.1),
        lambda: icp.registration_icp(src, tgt, 0.0),
        lambda: icp.registration_icp(src, tgt, -1.0),
        lambda: icp.registration_icp(src, tgt, np.nan),
        lambda: icp.registration_icp(src, tgt, 0.1, estimation="plane"),
        lambda: icp.registration_icp(src, tgt, 0.1, init=np.eye(3)),
        lambda: icp.registration_icp(src, tgt, 0.1, init=RigidTransformation(np.eye(3), np.zeros(3), 2.0)),
        lambda: icp.registration_icp(src, tgt, 0.1, init=np.full((4, 4), np.inf)),
        lambda: icp.registration_icp(src, tgt, 0.1, max_iteration=-1),
        lambda: icp.registration_icp(src, tgt, 0.1, max_iteration=2.5),
        lambda: icp.registration_icp(src, tgt, 0.1, relative_rmse=np.nan),
        lambda: icp.registration_icp(src, tgt, 0.1, estimation="point_to_plane", target_normals=nrm[:-1]),
        lambda: icp.evaluate_registration(src, tgt, 0.0),
        lambda: icp.evaluate_registration(src, tgt, 0.1, transformation=np.eye(2)),
        lambda: icp.nearest_neighbour(src, tgt[:, :2]),
        lambda: icp.nearest_neighbour(src, tgt, max_distance=-2.0),
    ):
        with pytest.raises(ValueError):
            call()


def test_point_to_plane_without_normals_points_to_the_normal_estimation():
    src, tgt, _ = _pair()
    with pytest.raises(ValueError, match="estimate_normals"):
        icp.registration_icp(src, tgt, 0.1, estimation="point_to_plane")


def test_more_than_one_rank_is_refused(monkeypatch):
    from probreg_amd import dist as pdist

    src, tgt, _ = _pair()
    monkeypatch.setattr(pdist, "world", lambda: (0, 2))
    for call in (lambda: icp.registration_icp(src, tgt, 0.1), lambda: icp.evaluate_registration(src, tgt, 0.1),
                 lambda: icp.nearest_neighbour(src, tgt)):
        with pytest.raises(NotImplementedError):
            call()


def test_valid_input_reaches_the_library():
    """Without a GPU every entry raises ProbregHipError once validation has passed (no CPU fallback); with one it runs."""
    src, tgt, nrm = _pair()

    class Cloud(object):
        points, normals = tgt, nrm

    class Scaled(object):
        def transform(self, points):
            return 1.1 * points

    calls = (lambda: icp.evaluate_registration(src, tgt, 0.5, Scaled()),
             lambda: icp.evaluate_registration(src, tgt, 0.5, RigidTransformation(np.eye(3), np.zeros(3), 1.1)),
             lambda: icp.registration_icp(src, tgt, np.inf, init=np.eye(4)),
             lambda: icp.registration_icp(src, Cloud(), 0.5, init=RigidTransformation(), estimation="point_to_plane"),
             lambda: icp.evaluate_registration(src, tgt, 0.5),
             lambda: icp.nearest_neighbour(src, tgt, 0.5))
    for call in calls:
        if _lib.device_count() > 0:
            assert call() is not None
        else:
            with pytest.raises(_lib.ProbregHipError):
                call()


def test_open3d_and_scikit_learn_are_not_imported():
    import re

    text = open(icp.__file__).read()
    assert not re.search(r"^\s*(import|from)\s+(open3d|sklearn|scipy)\b", text, flags=re.M)
