"""CPU checks of tests/oracle_dense_solve.py: every case tests/test_dense_solve_gpu.py imports must be one on which two
independent float64 host solves agree - otherwise the case says nothing about a third solver.  The caps are on the
yardstick itself (relative max-norm disagreement of LU and the SPD / Woodbury form), on the oracle's float32 kernel matrix
(a plan's own matrix is within 1.2e-7 of it, test_nonrigid_lowrank_gpu.py::test_factor_reproduces_the_exact_kernel_matrix)."""
import numpy as np
import pytest

import oracle_dense_solve as od


@pytest.mark.parametrize("case", od.NONRIGID_CASES, ids=od.case_id)
def test_nonrigid_host_solves_agree(case):
    ref = od.nonrigid_reference_f32(case)
    cap = od.Y_CAP_TINY_ALPHA if case.alpha is not None and case.alpha <= 1e-8 else od.Y_CAP
    print("y(W) = %.1e  y(G W) = %.1e  y(sigma2) = %.1e  unrefined W %.1e" % (ref.y_w, ref.y_disp, ref.y_sigma2,
                                                                            ref.y_w_unrefined))
    assert ref.y_w <= cap and ref.y_disp <= cap and ref.y_sigma2 <= cap
    assert ref.sigma2 > 0.0 and np.all(np.isfinite(ref.w))


@pytest.mark.parametrize("case", od.CONSTRAINED_CASES, ids=od.case_id)
def test_constrained_cases_on_the_exact_kernel(case):
    """The low-rank path is compared on the exact float64 kernel: same caps there."""
    inp = od.nonrigid_inputs(case)
    ref = od.nonrigid_reference(inp, od.kernel_exact(inp))
    cap = od.Y_CAP_TINY_ALPHA if case.alpha <= 1e-8 else od.Y_CAP
    assert ref.y_w <= cap and ref.y_disp <= cap and ref.y_sigma2 <= cap


@pytest.mark.parametrize("case", od.BCPD_CASES, ids=od.case_id)
def test_bcpd_host_solves_agree(case):
    ref = od.bcpd_reference(case)
    print("y(diag Sigma) = %.1e  y(v_hat) = %.1e" % (ref.y_sigma_diag, ref.y_v_hat))
    assert ref.y_sigma_diag <= od.Y_CAP and ref.y_v_hat <= od.Y_CAP


def test_case_list_covers_every_schedule_class():
    """One size per row of the look-ahead schedule (block rows 1, 2-4, 5-8, 9-12, >= 13), both ragged roundings of a last
    block, exact block / panel multiples, one real row in a last block; BCPD beyond 17 and 18 block rows."""
    nblk = {-(-c.m // 128) for c in od.DENSE_CASES}
    assert 1 in nblk and nblk & {2, 3, 4} and nblk & {5, 6, 7, 8} and nblk & {9, 10, 11, 12} and max(nblk) >= 13
    sizes = {c.m for c in od.DENSE_CASES}
    assert any(m < 128 and m % 8 for m in sizes) and any(m < 128 and m % 8 and -(-m // 8) * 8 == 128 for m in sizes)
    assert {128, 512, 1024, 1025} <= sizes
    assert {c.state for c in od.DENSE_CASES} == {"init", "late"}
    assert od.ORDER_CASE in od.DENSE_CASES
    assert max(-(-c.m // 128) for c in od.BCPD_CASES) >= 18


def test_the_constrained_case_tells_a_missing_refinement_from_a_working_one():
    """alpha = 1e-8: without its two refinement steps the SPD form is beyond the bound a solver is held to, by a wide
    margin - so a solver that skips them fails - and with them it is inside."""
    for case in od.CONSTRAINED_CASES:
        if case.alpha > 1e-8:
            continue
        ref = od.nonrigid_reference_f32(case)
        assert ref.y_w_unrefined > 10.0 * od.bound(ref.y_w, case.m), (case, ref.y_w_unrefined, ref.y_w)


@pytest.mark.parametrize("case", od.CONSTRAINED_CASES, ids=od.case_id)
def test_the_constrained_systems_have_an_spd_form(case):
    """The float32 kernel matrix is positive semi-definite only to ~1e-7, and the prior rows multiply it by
    sigma2 / alpha = 4.5e7: S = c I + D^1/2 G D^1/2 stays positive definite only while the paired source points are
    distinct enough for their 25 x 25 block of G to keep its smallest eigenvalue above that noise.  The seeded pairs do
    (a Cholesky-based solver has something to factor), with a margin that is checked here."""
    inp = od.nonrigid_inputs(case)
    d, c, _ = od.nonrigid_system(inp)
    sd = np.sqrt(d)
    s = sd[:, None] * od.kernel_f32(inp) * sd[None, :] + c * np.identity(case.m)
    assert np.linalg.eigvalsh(s)[0] > 0.5 * c


def test_the_inputs_are_what_the_plan_will_hold():
    """Clouds are float32 values (the plan stores float32), zeroed rows are exactly zero, the planar case is planar."""
    for case in (od.DENSE_CASES[0], od.ZERO_ROW_CASES[0], od.PLANAR_CASE, od.CONSTRAINED_CASES[0]):
        inp = od.nonrigid_inputs(case)
        assert np.array_equal(inp.y, inp.y.astype(np.float32).astype(np.float64))
        assert np.array_equal(inp.x, inp.x.astype(np.float32).astype(np.float64))
        assert inp.y.shape == (case.m, case.dim) and inp.x.shape == (case.m + 150, case.dim)
        if case.zero_rows:
            z = inp.p1 == 0.0
            assert z.sum() >= case.m // 10 and not np.any(inp.px[z])
        if case.alpha is not None:
            assert inp.p1_tilde.sum() == od.N_PAIRS
    b = od.bcpd_inputs(od.BCPD_CASES[0])
    assert np.count_nonzero(b.nu == 0.0) == b.nu.size // 12


def test_bound_is_the_stated_rule():
    assert od.bound(0.0, 1024) == 8.0 * 1024 * 2.0 ** -53
    assert od.bound(1e-9, 1024) == 8e-9
