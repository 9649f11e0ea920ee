"""Support-vector registration end to end on the GPU against the reference's own drivers, recorded in
tests/golden/svr_golden.npz by tests/golden/make_svr_golden.py.  Fixture-only."""
import os

import numpy as np
import pytest

import svr_cases as sc
from conftest import GOLDEN_DIR, Golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return Golden(os.path.join(GOLDEN_DIR, "svr_golden.npz"))


def test_fixture_has_three_rigid_seeds_within_half_the_tolerances(golden):
    seeds = golden.group("rigid")
    assert len(seeds) == 3
    for s in seeds:
        case = golden.case("rigid/" + s)
        e_true = sc.mat2euler(sc.rigid_case(int(case["seed"]))[2])
        assert np.all(case["ref_euler_err"] <= 0.5 * (0.1 + 0.1 * np.abs(e_true)))
        assert np.all(case["ref_t_err"] <= 0.5 * 1.0e-2)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_rigid_registration_recovers_the_rotation(golden, which):
    """The reference's tests/test_svr.py with its tolerances, on a synthetic surface."""
    from probreg_amd import l2dist_regs

    case = golden.case("rigid/" + golden.group("rigid")[which])
    src, tgt, rot = sc.rigid_case(int(case["seed"]))
    res = l2dist_regs.registration_svr(src, tgt)
    got, want = sc.mat2euler(res.rot), sc.mat2euler(rot)
    print("seed %d: euler error %s (reference %s), translation %s (reference %s)"
          % (case["seed"], np.abs(got - want), case["ref_euler_err"], np.abs(res.t), case["ref_t_err"]))
    assert np.allclose(got, want, atol=1.0e-1, rtol=1.0e-1)
    assert np.allclose(res.t, np.zeros(3), atol=1.0e-2, rtol=1.0e-3)


def test_tps_registration_moves_the_source_onto_the_target(golden):
    from probreg_amd import l2dist_regs, math_utils

    case = golden.case("tps/s500")
    src, tgt = sc.tps_case()
    reg = l2dist_regs.TPSSVR(src)
    n_sv = reg._feature_gen.support_vectors_.shape[0]
    assert np.array_equal(reg._cost_fn._control_pts, reg._feature_gen.support_vectors_)
    res = reg.registration(tgt)
    res2 = l2dist_regs.registration_svr(src, tgt, "nonrigid")
    assert res.control_pts.shape == (n_sv, 3) and res2.control_pts.shape == (n_sv, 3)
    assert np.array_equal(res.transform(src), res2.transform(src))
    before, after = math_utils.compute_rmse(src, tgt), math_utils.compute_rmse(res.transform(src), tgt)
    print("tps: %d control points (reference %d), rmse before %.5f after %.5f (reference %.5f)"
          % (n_sv, case["ref_n_control"], before, after, case["ref_rmse_after"]))
    assert abs(before - case["rmse_before"]) <= 1.0e-6
    assert after < before
    assert after < 2.0 * case["ref_rmse_after"]


def test_annealing_multiplies_gamma_and_leaves_the_feature_sigma(monkeypatch):
    from probreg_amd import l2dist_regs, svm, synthetic

    src = synthetic.surface(300, 5)
    tgt = src @ synthetic.rot_zx(10.0, 5.0).T
    gammas = []
    solve = svm.OcsvmPlan.solve

    def spy(self, gamma, nu, *a, **kw):
        gammas.append((gamma, nu))
        return solve(self, gamma, nu, *a, **kw)

    monkeypatch.setattr(svm.OcsvmPlan, "solve", spy)
    reg = l2dist_regs.RigidSVR(src)
    sigma0 = sc.estimate_sigma(src)
    gamma0 = 1.0 / (2.0 * sigma0 ** 2)
    assert reg._sigma == pytest.approx(sigma0, rel=1e-14) and reg._feature_gen._sigma == reg._sigma
    assert reg._feature_gen._gamma == pytest.approx(gamma0, rel=1e-14) and reg._feature_gen._nu == 0.1
    reg.registration(tgt, maxiter=2, tol=-1.0)
    g0 = 1.0 / (2.0 * reg._feature_gen._sigma ** 2)
    assert gammas == [(g0, 0.1), (g0, 0.1), (g0 * 10.0, 0.1), (g0 * 10.0, 0.1)]
    assert reg._sigma == pytest.approx(sigma0 * 0.9 * 0.9, rel=1e-14)  # the driver's sigma shrinks by its own delta
    assert reg._feature_gen._sigma == pytest.approx(sigma0, rel=1e-14)  # the feature generator's is not annealed
    assert reg._feature_gen._gamma == pytest.approx(gamma0 * 100.0, rel=1e-14)
