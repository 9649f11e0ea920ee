"""tests/oracle_ocsvm.py (the NumPy restatement of the one-class SVM solve, the yardstick of tests/test_ocsvm_gpu.py)
against scikit-learn's recorded solutions (tests/golden/svr_golden.npz), with the inequalities the GPU tests use
(tests/svr_cases.py check_solution).  No GPU, no scikit-learn."""
import os

import numpy as np
import pytest

import oracle_ocsvm as oc
import svr_cases as sc
from conftest import GOLDEN_DIR, Golden


@pytest.fixture(scope="module")
def golden():
    return Golden(os.path.join(GOLDEN_DIR, "svr_golden.npz"))


ALL_CASES = list(sc.SOLVER_CASES) + ["q_minus_1", "q_exact", "q_plus_1"]
RUNS = [(c, 1.0e-5) for c in ALL_CASES] + [(c, 1.0e-3) for c in sc.DEFAULT_TOL_CASES]


def test_fixture_holds_every_case_and_the_library_working_set_size(golden):
    from probreg_amd import svm

    assert sorted(golden.group("ocsvm")) == sorted(ALL_CASES)
    q = svm.working_set_size()
    assert int(golden._z["ocsvm_working_set_size"]) == q
    for name, (spec, _, _) in sc.working_set_cases(q).items():
        assert [str(s) for s in golden.case("ocsvm/" + name)["spec"]] == [str(s) for s in spec]


def test_recorded_solutions_are_what_the_helpers_say(golden):
    """objective / decision / rho / kkt_gap on scikit-learn's own alpha reproduce what scikit-learn reported."""
    for name in ALL_CASES:
        case = golden.case("ocsvm/" + name)
        x, gamma, nu, pts = sc.case_inputs(case)
        a = case["alpha"]
        assert abs(oc.objective(x, gamma, a) - case["objective"]) <= 1e-12 * abs(case["objective"]), name
        f = oc.decision(x, gamma, a, pts)
        assert np.max(np.abs(f - case["f_probe"])) <= 1e-12 * np.max(np.abs(case["f_probe"])), name
        assert np.max(np.abs(oc.decision(x, gamma, a, x) - oc.gradient(x, gamma, a))) <= 1e-12 * np.max(f), name
        if name == "c8_s64_nu1":
            assert oc.kkt_gap(x, gamma, a) == -np.inf and oc.rho(x, gamma, a) == np.inf
        else:
            # libsvm keeps Q in float32: each of its gradients, a sum of a_i Q_ij with sum a_i = nu n, is off by up to
            # nu n 2^-24, so its tol = 1e-7 holds in fp64 within twice that, and its rho (a mean of gradients) within once
            slack = nu * x.shape[0] * 2.0 ** -24
            assert oc.kkt_gap(x, gamma, a) < 1.0e-7 + 2.0 * slack, name
            assert abs(oc.rho(x, gamma, a) - case["rho"]) <= 1.0e-7 + slack, name


@pytest.mark.parametrize("name,tol", RUNS)
def test_smo_meets_the_bounds(golden, name, tol):
    case = golden.case("ocsvm/" + name)
    x, gamma, nu, _ = sc.case_inputs(case)
    alpha, steps, converged = oc.smo(x, gamma, nu, tol)
    assert converged
    sc.check_solution(case, x, gamma, nu, tol, alpha, label="smo " + name)
    if name == "c8_s64_nu1":
        assert steps == 0 and np.all(alpha == 1.0)


@pytest.mark.parametrize("name", ["c1_s300", "c5_s301_fractional", "c6_s257_2d", "c7_s150_twice", "c8_s64_nu1",
                                  "c9_s64_nu05", "q_minus_1", "q_exact", "q_plus_1"])
def test_working_set_decomposition_meets_the_bounds(golden, name):
    case = golden.case("ocsvm/" + name)
    x, gamma, nu, _ = sc.case_inputs(case)
    q = int(golden._z["ocsvm_working_set_size"])
    alpha, rounds, steps, converged, gap = oc.working_set_solve(x, gamma, nu, 1.0e-5, q_size=q)
    assert converged and gap < 1.0e-5
    sc.check_solution(case, x, gamma, nu, 1.0e-5, alpha, label="working set " + name)
    if name == "c8_s64_nu1":
        assert rounds == 0
    # a capped solve: feasible, not converged, no worse than the start
    a1, r1, _, c1, _ = oc.working_set_solve(x, gamma, nu, 1.0e-5, max_iter=1, q_size=q)
    if name != "c8_s64_nu1":
        assert r1 == 1 and not c1
        assert abs(a1.sum() - nu * x.shape[0]) <= 1e-9 * nu * x.shape[0] and a1.min() >= 0.0 and a1.max() <= 1.0
        assert oc.objective(x, gamma, a1) <= oc.objective(x, gamma, oc.initial_alpha(x.shape[0], nu))


def test_working_set_holds_the_maximal_violating_pair_and_no_duplicates():
    rng = np.random.RandomState(3)
    for n, q in [(1000, 256), (255, 256), (130, 256), (7, 8)]:
        alpha = rng.choice([0.0, 1.0, 0.3, 0.7], n)
        grad = rng.standard_normal(n)
        grad[rng.randint(0, n, 5)] = grad[0]  # ties
        ws = oc.select_working_set(alpha, grad, q)
        live = ws[ws >= 0]
        assert live.size == np.unique(live).size
        up, low = alpha < 1.0, alpha > 0.0
        assert int(np.argmax(np.where(up, -grad, -np.inf))) in live
        assert np.max(grad[live][alpha[live] > 0.0]) == np.max(grad[low])
        assert oc.gap_of(alpha[live], grad[live]) == oc.gap_of(alpha, grad)
