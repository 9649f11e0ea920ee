"""The blocked fp64 Cholesky solves of spd_solve.hip through their drivers (cpd_nonrigid_solve.hip, cpd_bcpd_solve.hip), one
M-step / one solve at a time, against LAPACK on the same
matrix - per class of the look-ahead schedule (which kernels and streams run depends on ceil(M / 128) alone):

  block rows   M             what runs
  1            <= 128        k_potrf_inv only; the ragged block rounds its active part up to a multiple of 8
  2 - 4        129 - 512     one outer panel: panel solve (mode 0) and in-panel update (mode 2)
  5 - 8        513 - 1024    two outer panels, U1 on the plan stream, side stream idle
  9 - 12       1025 - 1536   first U2 on the side stream (triangular mode 1 grid)
  >= 13        >= 1537       a second U2 queued behind the first, U1(J) waits for U2(J-1)
  BCPD: the K-deep left update of the many-right-hand-side solve first runs at 17 block rows (M >= 2049), the update inside
  a second panel at 18 (M >= 2177).

The plan is driven directly (set_source, build_g, moments_from_estep with the HOST oracle's E-step arrays, set_params,
mstep_nonrigid), so only the M-step is compared.  The reference is LAPACK LU in float64 on the float32 matrix the plan
itself holds (get_g), and the bound of every quantity is tests/oracle_dense_solve.py's

    8 * max(y, M * 2^-53)      y = what a second, independent float64 host solve leaves against the first

relative to the reference's largest entry - nothing is measured against the code under test.  On the low-rank path the
reference uses the exact float64 kernel and the bound for W is test_nonrigid_lowrank_gpu.py's 1e-7 (the factor is cut at
1e-14 per entry) unless the yardstick bound is larger.

Measured on the MI355X (y: host yardstick, gpu: error of the HIP path against solve 1; W / G W / sigma2):
  path / case                                  y(W)     gpu(W)   y(G W)   gpu(G W) y(s2)    gpu(s2)
  dense m100-init                              2.3e-13  7.5e-14  9.8e-15  7.5e-15  1.7e-16  3.5e-16
  dense m100-late                              3.1e-11  1.4e-11  3.2e-11  3.6e-11  6.9e-13  2.4e-13
  dense m121-init                              2.3e-13  1.4e-13  1.1e-14  6.8e-15  1.8e-16  1.8e-16
  dense m121-late                              5.0e-11  2.8e-11  4.2e-11  2.2e-11  2.7e-13  1.6e-12
  dense m128-init                              1.7e-13  2.1e-13  5.3e-15  2.7e-14  0.0e+00  3.6e-16
  dense m128-late                              4.4e-11  2.2e-11  6.2e-11  7.0e-11  9.4e-13  2.1e-12
  dense m300-init                              6.0e-13  1.6e-13  1.4e-14  9.3e-15  0.0e+00  1.8e-16
  dense m300-late                              1.7e-10  1.4e-10  2.3e-10  3.1e-10  3.0e-12  1.6e-12
  dense m512-init                              1.1e-12  3.0e-13  2.2e-14  1.1e-14  0.0e+00  0.0e+00
  dense m512-late                              1.4e-10  1.2e-10  3.3e-10  7.7e-10  6.9e-13  1.9e-13
  dense m777-init                              1.7e-12  5.5e-13  3.0e-14  2.4e-14  1.8e-16  1.8e-16
  dense m777-late                              3.9e-10  6.3e-10  2.9e-10  7.4e-10  7.3e-12  1.2e-12
  dense m1024-init                             4.0e-12  1.1e-12  4.7e-14  8.6e-14  0.0e+00  1.8e-16
  dense m1024-late                             6.3e-10  6.0e-10  2.6e-10  2.3e-10  1.7e-12  2.5e-15
  dense m1025-init                             2.6e-12  7.5e-13  2.4e-14  1.1e-13  0.0e+00  3.5e-16
  dense m1025-late                             1.2e-09  6.8e-10  2.5e-10  2.2e-10  4.6e-12  3.0e-12
  dense m1100-init                             4.3e-12  8.3e-13  5.4e-14  4.3e-14  1.8e-16  0.0e+00
  dense m1100-late                             9.6e-10  7.8e-10  2.1e-10  3.0e-10  9.3e-13  4.2e-12
  dense m1700-init                             5.4e-12  1.4e-12  3.8e-14  3.6e-14  1.8e-16  0.0e+00
  dense m1700-late                             1.0e-09  5.2e-10  3.2e-10  2.3e-10  5.2e-12  5.3e-13
  zerorows m300-init-zerorows                  3.6e-13  1.7e-13  1.5e-14  2.9e-14  0.0e+00  0.0e+00
  zerorows m300-late-zerorows                  1.9e-10  1.5e-10  1.0e-10  1.9e-10  3.8e-14  6.6e-14
  zerorows m1100-init-zerorows                 2.3e-12  8.1e-13  3.9e-14  2.5e-14  0.0e+00  0.0e+00
  zerorows m1100-late-zerorows                 8.2e-10  5.0e-10  3.4e-10  7.0e-10  3.7e-14  1.3e-13
  unsorted m1100-late                          9.6e-10  7.6e-10  2.1e-10  2.4e-10  9.3e-13  1.7e-12
  sorted m1100-late                            9.6e-10  7.8e-10  2.1e-10  3.0e-10  9.3e-13  4.2e-12
  planar m300-late-d2                          2.7e-10  3.4e-10  3.7e-10  9.0e-10  2.4e-12  1.4e-12
  constrained m300-init-alpha0.01              1.9e-13  1.5e-13  7.3e-14  5.2e-14  6.4e-15  3.5e-16
  constrained m300-init-alpha1e-08             8.3e-11  1.3e-10  6.0e-11  1.5e-10  2.0e-11  7.0e-11
  constrained m1100-init-alpha0.01             1.5e-13  1.4e-13  4.1e-13  2.7e-13  1.6e-14  1.2e-14
  constrained m1100-init-alpha1e-08            5.8e-09  3.5e-09  5.7e-09  2.3e-09  3.5e-09  1.9e-09
  constrained-lowrank m300-init-alpha0.01      5.9e-14  9.2e-14  -        -        -        -
  constrained-lowrank m300-init-alpha1e-08     1.1e-10  5.7e-10  -        -        -        -
  constrained-lowrank m1100-init-alpha0.01     1.1e-13  2.2e-13  -        -        -        -
  constrained-lowrank m1100-init-alpha1e-08    3.9e-09  4.6e-09  -        -        -        -
  after-pivot-error m300-late                  1.7e-10  1.4e-10  2.3e-10  3.1e-10  3.0e-12  1.6e-12
  lowrank-after-pivot-error m1100-init         4.3e-12  8.1e-14  -        -        -        -
  BCPD case                                    y(diag Sigma) gpu     y(v_hat) gpu
  m100-cfac37.5                                9.7e-16       7.5e-16 2.7e-14  2.5e-14
  m100-cfac40000                               1.0e-15       7.7e-16 2.0e-11  2.4e-11
  m1100-cfac37.5                               2.5e-15       1.5e-15 6.8e-14  2.5e-14
  m1100-cfac40000                              3.7e-15       2.6e-15 1.1e-10  3.5e-11
  m2300-cfac37.5                               2.5e-15       4.6e-15 9.0e-14  2.9e-14
  m2300-cfac40000                              2.9e-15       4.4e-15 3.3e-10  3.3e-11

What these tests found when they were written (figures of the code before its fix, same columns):
  * G W of the late state at one block row: 5.2e-10 / 7.2e-10 / 1.3e-9 at M = 100 / 121 / 128 against limits of 2.6e-10 /
    3.3e-10 / 5.0e-10, with W itself inside (1.4e-11).  The triangular sweeps multiplied by the explicit inverse of each
    128 x 128 diagonal block, which is only conditionally stable; a float64 host model of exactly that (LAPACK factor, block
    inverses) gives 3.3e-10 / 5.7e-10 at M = 100 / 128, substitution 4.4e-11 / 6.0e-11.  k_diag_solve now refines once against
    the factor (host model 2.1e-11 / 3.8e-11, measured above).
  * BCPD: 6e-8 .. 1e-6 in both quantities at every size - float32 ulps of G, not round-off of the solve: the square root of
    the inverse-multiquadric kernel was the hardware estimate.  It is correctly rounded now and the plan's matrix is the
    oracle's bit for bit (which is why the oracle's matrix can be the reference's here).
What they cannot see: the second Newton step of rsqrt_newton.  The hardware estimate is good to 2^-26, so one step leaves
1.5 * 2^-52 - a pivot off by an ulp and a half, the size of the rounding of S's own entries; with one step every figure above
stays inside its limit (largest ratio 0.65).  Without refinement steps test_constrained_mstep_dense[...alpha1e-08] fails
(1e-7 .. 2e-6 in W); without the K-deep left update test_bcpd_solve[m2300-...] fails.
"""
import numpy as np
import pytest

import oracle_dense_solve as od

pytestmark = pytest.mark.gpu

LOWRANK_W_BOUND = 1e-7   # tests/test_nonrigid_lowrank_gpu.py::test_lowrank_mstep_equals_fp64_solve_on_the_exact_matrix
DENSE = (0, 0, 0.0)
# factor at its limit (1e-14 per entry).  The default rank cap is M / 2: 150 at M = 300, a dozen columns short of what this
# kernel (beta = 2 on a unit-sized cloud) needs at 1e-14 - so the cap is given
LOWRANK = (1, 256, 1e-14)

_references = {}


def _open_plan(inp, solver, sort_source=True):
    from probreg_amd import engine

    plan = engine.CpdPlan()
    try:
        plan.set_options(sort_source=sort_source, sort_target=True, cull=True)
        plan.set_source(inp.y)
        plan.set_target(inp.x)
        plan.set_nonrigid_solver(*solver)
        plan.build_g(inp.beta)
        plan.init_sums()
        plan.init_params()
        if inp.alpha is not None:
            plan.set_priors(inp.p1_tilde, inp.px_tilde, inp.alpha)
    except Exception:
        plan.close()
        raise
    return plan


def _mstep(plan, inp, p1=None, px=None, sigma2_prev=None):
    from probreg_amd import _lib

    plan.moments_from_estep(inp.pt1, inp.p1 if p1 is None else p1, inp.px if px is None else px)
    p = np.zeros(_lib.PRG_NPARAMS)
    p[0] = p[4] = p[8] = p[12] = 1.0
    p[13] = inp.sigma2_prev if sigma2_prev is None else sigma2_prev
    plan.set_params(p)
    plan.mstep_nonrigid(inp.lmd)


def _reference(case, plan, exact=False):
    """Solve 1 and the yardsticks of a case, computed once: on the plan's own float32 matrix (the same for every plan of
    that cloud: an entry depends on its two points alone), or on the exact float64 kernel for the low-rank path."""
    key = (case, exact)
    if key not in _references:
        inp = od.nonrigid_inputs(case)
        g = od.kernel_exact(inp) if exact else plan.get_g().astype(np.float64)
        _references[key] = od.nonrigid_reference(inp, g)
    return _references[key]


def _compare(case, plan, ref, tag, floor=0.0, quantities=("w", "disp", "sigma2")):
    """Print every figure, then hold each to max(floor, 8 * max(y, M * 2^-53))."""
    inp = od.nonrigid_inputs(case)
    got = {"w": (od.rel_max(plan.get_w(), ref.w), ref.y_w),
           "disp": (od.rel_max(plan.nonrigid_apply() - inp.y, ref.disp), ref.y_disp),
           "sigma2": (abs(plan.get_params()[13] - ref.sigma2) / abs(ref.sigma2), ref.y_sigma2)}
    bad = []
    for q in quantities:
        err, y = got[q]
        limit = max(floor, od.bound(y, case.m))
        print("DENSE_SOLVE %s %s %s y=%.1e gpu=%.1e limit=%.1e" % (tag, od.case_id(case), q, y, err, limit))
        if not err <= limit:
            bad.append((q, err, limit))
    assert not bad, (od.case_id(case), tag, bad)


def _run_dense(case, sort_source=True, tag="dense"):
    inp = od.nonrigid_inputs(case)
    plan = _open_plan(inp, DENSE, sort_source)
    try:
        assert plan.nonrigid_rank() == 0
        ref = _reference(case, plan)
        _mstep(plan, inp)
        _compare(case, plan, ref, tag)
    finally:
        plan.close()


@pytest.mark.parametrize("case", od.DENSE_CASES, ids=od.case_id)
def test_dense_mstep_per_schedule_class(case):
    _run_dense(case)


@pytest.mark.parametrize("case", od.ZERO_ROW_CASES, ids=od.case_id)
def test_rows_without_support(case):
    """A tenth of the rows has p1 = 0 and px = 0 exactly: sp = 0 there and the row of S is c e_i."""
    inp = od.nonrigid_inputs(case)
    assert np.count_nonzero(inp.p1 == 0.0) >= case.m // 10
    _run_dense(case, tag="zerorows")


@pytest.mark.parametrize("sort_source", [False, True], ids=["unsorted", "sorted"])
def test_results_come_back_in_the_callers_order(sort_source):
    """The plan sorts the source along a space-filling curve unless told not to; W, G W and sigma2 must match the same
    reference, in the caller's point order, either way."""
    _run_dense(od.ORDER_CASE, sort_source=sort_source, tag="sorted" if sort_source else "unsorted")


def test_planar_cloud():
    """D = 2: the third right-hand side of the [mp][3] vectors stays zero and sigma2 divides by n_p * 2."""
    inp = od.nonrigid_inputs(od.PLANAR_CASE)
    assert inp.y.shape[1] == 2
    _run_dense(od.PLANAR_CASE, tag="planar")


@pytest.mark.parametrize("case", od.CONSTRAINED_CASES, ids=od.case_id)
def test_constrained_mstep_dense(case):
    """Correspondence priors scale 25 rows by sigma2 / alpha: at alpha = 1e-8 the push-through form alone is 1e-7 .. 2e-6
    from LU (oracle_dense_solve: y_w_unrefined) and two refinement steps bring it back to the yardstick."""
    _run_dense(case, tag="constrained")


@pytest.mark.parametrize("case", od.CONSTRAINED_CASES, ids=od.case_id)
def test_constrained_mstep_lowrank(case):
    inp = od.nonrigid_inputs(case)
    plan = _open_plan(inp, LOWRANK)
    try:
        assert plan.nonrigid_rank() > 0
        ref = _reference(case, plan, exact=True)
        _mstep(plan, inp)
        _compare(case, plan, ref, "constrained-lowrank", floor=LOWRANK_W_BOUND, quantities=("w",))
    finally:
        plan.close()


# ---- BCPD ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", od.BCPD_CASES, ids=od.case_id)
def test_bcpd_solve(case):
    """prg_cpd_bcpd_solve; cfac = 4e4 is s^2 / sigma2^2 of a late iteration, where lmd / cfac is small against the largest
    eigenvalue of D^1/2 G D^1/2.  The plan's inverse-multiquadric matrix is the oracle's bit for bit (float32, every
    operation correctly rounded, same order), so the oracle's matrix is the reference's."""
    from probreg_amd import engine

    inp = od.bcpd_inputs(case)
    ref = od.bcpd_reference(case)
    plan = engine.CpdPlan()
    try:
        plan.set_source(inp.src)
        plan.bcpd_build_g(1.0)
        v, sd = plan.bcpd_solve(inp.lmd, inp.cfac, inp.resid, inp.nu)
    finally:
        plan.close()
    bad = []
    for q, got, want, y in (("sigma_diag", sd, ref.sigma_diag, ref.y_sigma_diag), ("v_hat", v, ref.v_hat, ref.y_v_hat)):
        err, limit = od.rel_max(got, want), od.bound(y, case.m)
        print("DENSE_SOLVE bcpd %s %s y=%.1e gpu=%.1e limit=%.1e" % (od.case_id(case), q, y, err, limit))
        if not err <= limit:
            bad.append((q, err, limit))
    assert not bad, (od.case_id(case), bad)


# ---- non-positive pivots --------------------------------------------------------------------------------------------------
def _mstep_without_support(plan, inp):
    """p1 = 0 and px = 0 everywhere and sigma2_prev = -1: the system matrix is c I with c = -lmd, every pivot negative."""
    _mstep(plan, inp, p1=np.zeros_like(inp.p1), px=np.zeros_like(inp.px), sigma2_prev=-1.0)


def test_dense_path_reports_a_non_positive_pivot_and_stays_usable():
    from probreg_amd import _lib

    case = od.DENSE_CASES[od.SCHEDULE_SIZES.index(300) * 2 + 1]
    assert case == od.NonrigidCase(300, "late", False, 3, None)
    inp = od.nonrigid_inputs(case)
    plan = _open_plan(inp, DENSE)
    try:
        ref = _reference(case, plan)
        with pytest.raises(_lib.ProbregHipError, match="not positive definite at pivot"):
            _mstep_without_support(plan, inp)
        _mstep(plan, inp)
        _compare(case, plan, ref, "after-pivot-error")
    finally:
        plan.close()


def test_lowrank_path_reports_a_non_positive_pivot_once_and_stays_usable():
    """The low-rank M-step does not stall the stream to look at its pivot flag: the M-step returns, the next get_params
    reports the failure - once."""
    from probreg_amd import _lib

    case = od.DENSE_CASES[od.SCHEDULE_SIZES.index(1100) * 2]
    assert case == od.NonrigidCase(1100, "init", False, 3, None)
    inp = od.nonrigid_inputs(case)
    plan = _open_plan(inp, LOWRANK)
    try:
        assert plan.nonrigid_rank() > 0
        _mstep_without_support(plan, inp)
        with pytest.raises(_lib.ProbregHipError, match="not positive definite at pivot"):
            plan.get_params()
        plan.get_params()
        ref = _reference(case, plan, exact=True)
        _mstep(plan, inp)
        _compare(case, plan, ref, "lowrank-after-pivot-error", floor=LOWRANK_W_BOUND, quantities=("w",))
    finally:
        plan.close()
