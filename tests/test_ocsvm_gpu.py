"""The one-class SVM solve on the GPU (csrc/ocsvm.hip through ``probreg_amd.svm``) against scikit-learn's recorded
solutions (tests/golden/svr_golden.npz).  Fixture-only: nothing here needs scikit-learn.

Two tol-optimal solutions of an ill-conditioned Q differ in single alpha_i and in the support set (scikit-learn against
itself at tol 1e-3 against 1e-7: 0.23 in one alpha_i in case c6, 0.13 in c3, 62 support vectors in c4; the fixture's
``sklearn_tol_info``), so alpha and
the support set are not compared to the fixture.  Compared is what the problem determines: feasibility, the stop test,
the objective, the decision function and rho, with the derived bounds of tests/svr_cases.py check_solution, every
quantity recomputed from the returned alpha by tests/oracle_ocsvm.py (itself tied to the fixture by
tests/test_oracle_ocsvm.py).
"""
import os

import numpy as np
import pytest

import oracle_ocsvm as oc
import svr_cases as sc
from conftest import GOLDEN_DIR, Golden

pytestmark = pytest.mark.gpu

ALL_CASES = list(sc.SOLVER_CASES) + ["q_minus_1", "q_exact", "q_plus_1"]
RUNS = [(c, 1.0e-5) for c in ALL_CASES] + [(c, 1.0e-3) for c in sc.DEFAULT_TOL_CASES]


@pytest.fixture(scope="module")
def golden():
    return Golden(os.path.join(GOLDEN_DIR, "svr_golden.npz"))


def raw_solve(x, gamma, nu, tol, **kw):
    from probreg_amd import svm

    plan = svm.OcsvmPlan()
    plan.set_data(x)
    stats = plan.solve(gamma, nu, tol, **kw)
    return plan, stats


@pytest.mark.parametrize("name,tol", RUNS)
def test_solution_against_scikit_learn(golden, name, tol):
    from probreg_amd import svm

    case = golden.case("ocsvm/" + name)
    x, gamma, nu, pts = sc.case_inputs(case)
    sigma = sc.estimate_sigma(x)
    est = svm.OneClassSVM(x.shape[1], sigma, gamma=gamma, nu=nu, tol=tol)
    sv, w = est.compute(x)
    alpha, rho, obj, support = est._plan.solution()
    print("%s tol %.0e: rounds %d steps %d" % (name, tol, est.n_iter_, est.n_inner_iter_))
    assert est.converged_ and est.gap_ < tol
    # the support list, the coefficients and the feature weights are alpha on its non-zeros, ascending
    assert np.array_equal(support, np.flatnonzero(alpha)) and np.array_equal(est.support_, support)
    assert est.dual_coef_.shape == (1, support.size) and np.array_equal(est.dual_coef_[0], alpha[support])
    assert np.array_equal(sv, x[support]) and np.array_equal(est.support_vectors_, sv)
    assert np.array_equal(w, alpha[support] * np.power(2.0 * np.pi * sigma ** 2, x.shape[1] * 0.5))
    assert est.offset_.shape == (1,) and est.offset_[0] == rho
    # the decision sum of the library is the oracle's on the same alpha
    f_own, f_probe = est._plan.decision(x), est._plan.decision(pts)
    for got, at in ((f_own, x), (f_probe, pts)):
        want = oc.decision(x, gamma, alpha, at)
        assert np.max(np.abs(got - want)) <= 1.0e-12 * np.max(np.abs(want))
    assert np.array_equal(est.decision_function(pts), f_probe - rho)
    assert abs(obj - oc.objective(x, gamma, alpha)) <= 1.0e-12 * obj
    sc.check_solution(case, x, gamma, nu, tol, alpha, rho=rho, f_own=f_own, f_probe=f_probe, label=name)
    if np.isfinite(rho):
        assert abs(rho - oc.rho(x, gamma, alpha)) <= 1.0e-12 * abs(rho)
    # a second solve on a fresh handle through the raw calls: byte-identical
    plan, stats = raw_solve(x, gamma, nu, tol)
    alpha2, rho2, obj2, support2 = plan.solution()
    plan.close()
    assert stats == (est.n_iter_, est.n_inner_iter_, True, est.gap_)
    assert alpha2.tobytes() == alpha.tobytes() and rho2 == rho and obj2 == obj and np.array_equal(support2, support)


def test_nu_one_puts_every_alpha_at_the_bound(golden):
    case = golden.case("ocsvm/c8_s64_nu1")
    x, gamma, nu, _ = sc.case_inputs(case)
    plan, (rounds, steps, converged, gap) = raw_solve(x, gamma, nu, 1.0e-5)
    alpha, rho, obj, support = plan.solution()
    plan.close()
    assert np.all(alpha == 1.0) and rounds == 0 and steps == 0 and converged and gap == -np.inf
    assert np.array_equal(support, np.arange(x.shape[0])) and rho == np.inf  # libsvm's midpoint of (max G, +inf)


@pytest.mark.parametrize("name", ["c3_s2000", "c4_s2000_annealed", "q_plus_1"])
def test_capped_solve_returns_a_feasible_point(golden, name):
    case = golden.case("ocsvm/" + name)
    x, gamma, nu, _ = sc.case_inputs(case)
    n = x.shape[0]
    plan, (rounds, steps, converged, gap) = raw_solve(x, gamma, nu, 1.0e-5, max_iter=1)
    alpha = plan.solution()[0]
    plan.close()
    assert rounds == 1 and steps >= 1 and not converged and gap >= 1.0e-5
    assert np.all(alpha >= 0.0) and np.all(alpha <= 1.0) and abs(alpha.sum() - nu * n) <= 1.0e-9 * nu * n
    assert abs(gap - oc.kkt_gap(x, gamma, alpha)) <= 1.0e-9
    assert oc.objective(x, gamma, alpha) <= oc.objective(x, gamma, oc.initial_alpha(n, nu))
    # a step cap inside the round is honoured too, and a start that is not moved at all is reported as such
    plan, (rounds, steps, converged, _) = raw_solve(x, gamma, nu, 1.0e-5, max_iter=2, inner_cap=3)
    plan.close()
    assert rounds == 2 and steps == 6 and not converged
    plan, (rounds, steps, converged, _) = raw_solve(x, gamma, nu, 1.0e-5, max_iter=0)
    alpha0 = plan.solution()[0]
    plan.close()
    assert rounds == 0 and steps == 0 and not converged and np.array_equal(alpha0, oc.initial_alpha(n, nu))


def test_bad_arguments_raise_through_the_status_channel():
    from probreg_amd import _lib, svm, synthetic

    x = synthetic.surface(50, 0)
    plan = svm.OcsvmPlan()
    with pytest.raises(_lib.ProbregHipError):
        plan.solve(1.0, 0.1)  # no data yet
    for bad in (np.zeros((0, 3)), np.zeros((5, 4)), np.zeros((5, 1)), np.zeros(5)):
        with pytest.raises(ValueError):
            plan.set_data(bad)
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 1] = v
        with pytest.raises(ValueError):
            plan.set_data(y)
    plan.set_data(x)
    with pytest.raises(_lib.ProbregHipError):
        plan.solution()  # not solved yet
    with pytest.raises(_lib.ProbregHipError):
        plan.decision(x)
    for gamma, nu, tol in [(1.0, 0.0, 1e-3), (1.0, -0.1, 1e-3), (1.0, 1.5, 1e-3), (1.0, np.nan, 1e-3), (0.0, 0.1, 1e-3),
                           (-1.0, 0.1, 1e-3), (np.inf, 0.1, 1e-3), (np.nan, 0.1, 1e-3), (1.0, 0.1, 0.0), (1.0, 0.1, -1.0)]:
        with pytest.raises(ValueError):
            plan.solve(gamma, nu, tol)
    with pytest.raises(ValueError):
        plan.solve(1.0, 0.1, max_iter=-1)
    with pytest.raises(ValueError):
        plan.solve(1.0, 0.1, inner_cap=0)
    assert plan.solve(1.0, 0.1)[2]  # the handle is still usable
    with pytest.raises(ValueError):
        plan.decision(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        plan.decision(np.full((3, 3), np.nan))
    assert _lib.lib.prg_ocsvm_solve(None, 1.0, 0.1, 1e-3, 1, 1, None, None, None, None) == _lib.PRG_ERR_INVALID
    assert _lib.lib.prg_ocsvm_working_set_size(None) == _lib.PRG_ERR_INVALID
    plan.close()
    est = svm.OneClassSVM(3, 1.0, nu=2.0)
    with pytest.raises(ValueError):
        est.compute(x)
    with pytest.raises(ValueError):
        svm.OneClassSVM(3, 1.0).decision_function(x)


def test_one_point_and_profile():
    from probreg_amd import svm

    plan = svm.OcsvmPlan()
    plan.set_data(np.array([[0.5, -1.0]]))
    rounds, _, converged, _ = plan.solve(1.0, 0.5)
    alpha, rho, obj, support = plan.solution()
    assert converged and rounds == 0 and np.array_equal(alpha, [0.5]) and rho == 0.5 and obj == 0.125
    assert np.array_equal(plan.decision(np.array([[0.5, -1.0]])), [0.5])
    plan.set_profile(True)
    plan.solve(1.0, 0.5)
    assert plan.profile().shape == (4,) and np.all(plan.profile() >= 0.0)
    plan.close()


def test_a_capped_feature_fit_warns_and_still_returns_features(golden, caplog):
    import logging

    from probreg_amd import svm

    case = golden.case("ocsvm/c3_s2000")
    x, gamma, nu, _ = sc.case_inputs(case)
    est = svm.OneClassSVM(3, 1.0, gamma=gamma, nu=nu, max_iter=1)
    with caplog.at_level(logging.WARNING, logger="probreg"):
        sv, w = est.compute(x)
    assert not est.converged_ and est.n_iter_ == 1 and sv.shape[0] == w.shape[0] > 0
    assert any("max_iter" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="probreg"):
        svm.OneClassSVM(3, 1.0, gamma=gamma, nu=nu).compute(x)
    assert not caplog.records
