"""BCPD on the pivoted-Cholesky factor of its coherence kernel: prg_cpd_bcpd_set_solver, the factor of the
inverse-multiquadric kernel, prg_cpd_bcpd_solve on a plan that holds the factor, and CombinedBCPD(solver=...).

Round-off may order two nearly equal pivots differently from the restatement (tests/oracle_bcpd_lowrank.py), so F itself is
never compared: F F^T, v_hat and diag Sigma are.

Bounds
  factor       max |G - F F^T| <= tol, G evaluated in float64 on the float32 coordinates the plan holds.  F F^T is read off
               the plan by applying it to unit vectors (T = y + G W, prg_cpd_nonrigid_apply; y from W = 0).
  solve        against the restatement's low-rank solve with the same tol and the same point order (so the same pivots):
               8 * max(y, M 2^-53), y = the disagreement of two float64 host evaluations of that formula (LAPACK Cholesky
               against numpy.linalg.solve, independent of each other from the coordinates on: see the head of
               tests/oracle_bcpd_lowrank.py for why a shared factor measures the solver and not the formula) - the rule
               of tests/test_dense_solve_gpu.py;
               against the dense float64 form Sigma = G (lmd I + c D G)^-1: 4 * e_trunc + that allowance, e_trunc = what the
               restatement's own low-rank solve leaves against its dense one (tests/test_bcpd_lowrank_host.py prints it);
               the 4 covers another pivot order.
  registration TOL_T = 1e-4 of tests/test_bcpd_gpu.py: ten float32 E-steps, not the factor, set it (on the host the
               truncation alone moved T by 2.7e-10 after 10 iterations of the 900-point version of this pair).

Measured on MI355X (gfx950), BCPD_LOWRANK lines of this file (relative to the largest entry; M = 1500 unless said):
  factor        max |G - F F^T| 9.97e-12 at rank 507 (3-D, extent 2.2), 8.6e-12 at rank 153 (2-D), 9.2e-12 at rank 26 (extent 0.1),
                <= 2.2e-16 at M = 1, 2; copies: rank 237 of 257, 1.3e-15
  solve                          v_hat: y / vs low-rank / e_trunc / vs dense        diag Sigma: the same
    lmd 2  cfac 5                4.7e-13 / 4.2e-13 / 4.9e-10 / 4.9e-10              9.2e-14 / 1.4e-13 / 2.3e-10 / 2.3e-10
    lmd 2  cfac 1e3              3.4e-11 / 3.4e-11 / 3.4e-08 / 3.3e-08              2.3e-12 / 2.9e-12 / 6.6e-09 / 6.6e-09
    lmd 50 cfac 1e5              1.1e-10 / 1.2e-10 / 1.1e-07 / 1.1e-07              6.1e-12 / 7.2e-12 / 1.8e-08 / 1.8e-08
    one nu = 1e6                 5.1e-10 / 6.2e-10 / 3.2e-08 / 3.2e-08              3.3e-10 / 3.2e-10 / 6.6e-09 / 6.6e-09
    nu = 0 everywhere            0 / 0 / 0 / 0                                      4.3e-15 / 6.3e-15 / 1.0e-11 / 1.0e-11
    2-D                          3.5e-11 / 3.9e-11 / 4.7e-08 / 4.7e-08              3.3e-12 / 3.4e-12 / 1.5e-08 / 1.5e-08
    shuffled                     3.5e-11 / 3.5e-11 / 3.2e-08 / 3.2e-08              5.7e-12 / 7.8e-12 / 2.1e-08 / 2.1e-08
    rank 130 (tol 1e-5)          1.1e-11 / 1.4e-11 / 2.8e-02 / 2.8e-02              1.0e-12 / 1.2e-12 / 6.3e-03 / 6.3e-03
    rank 37, rank 1              2.4e-13 / 3.0e-13, 3.3e-16 / 6.7e-16               3.8e-14 / 3.4e-14, 4.9e-16 / 7.3e-16
    M 257, lmd 50 cfac 1e5       4.6e-12 / 6.2e-12 / 3.6e-09 / 3.6e-09              1.9e-13 / 3.4e-13 / 2.5e-09 / 2.5e-09
  With y taken from two solvers on ONE factor and one summation order (2e-14 .. 5e-11) the device was 3.4e-11 .. 6.2e-10 from
  evaluation 1 in v_hat and 12 cases of 22 missed; the host restatement moves by the same 3.4e-11 .. 5.8e-10 when the summation
  order of its own factor or Gram matrix changes, which is what y now contains.
  registration  T 5.2e-07 / rot 3.8e-10 / scale 2.9e-08 from the host's dense form, 2.4e-05 / 1.1e-09 / 8.8e-09 from the device's
                dense solver (limit 1e-4); two runs: identical bytes
"""
import numpy as np
import pytest

import oracle_bcpd_lowrank as ob

pytestmark = pytest.mark.gpu

TOL_T = 1e-4          # tests/test_bcpd_gpu.py
KERNEL_TOL = 1e-11    # the default of prg_cpd_bcpd_set_solver


def _open_plan(points, mode, max_rank=0, tol=0.0, sort_source=True):
    from probreg_amd import engine

    plan = engine.CpdPlan()
    try:
        plan.set_options(sort_source=sort_source, sort_target=True, cull=True)
        plan.set_source(points)
        plan.bcpd_set_solver(mode, max_rank, tol)
        plan.bcpd_build_g(1.0)
    except Exception:
        plan.close()
        raise
    return plan


def _product_with_kernel(plan):
    """F F^T (or the dense G) of a plan, M x M float64 in the caller's order: dim columns per apply."""
    m, dim = plan.m, plan.dim
    plan.set_w(np.zeros((m, dim)))
    y0 = plan.nonrigid_apply()
    out = np.empty((m, m))
    for j0 in range(0, m, dim):
        w = np.zeros((m, dim))
        cols = np.arange(j0, min(j0 + dim, m))
        w[cols, cols - j0] = 1.0
        plan.set_w(w)
        out[:, cols] = (plan.nonrigid_apply() - y0)[:, :cols.size]
    plan.set_w(np.zeros((m, dim)))
    return out


# ---- the factor -----------------------------------------------------------------------------------------------------------
def _factor_cloud(m, dim, scale):
    from probreg_amd import synthetic

    return np.ascontiguousarray(synthetic.surface(m, 100 + m)[:, :dim] * scale)


@pytest.mark.parametrize("scale", [0.05, 1.0], ids=["extent0.1", "extent2.2"])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("m", [1, 2, 255, 257, 1500])
def test_factor_reproduces_the_kernel(m, dim, scale):
    """Rank of a few tens at an extent of 0.1 and about 500 at 2.2 in 3-D (M = 1500: the factor buffer grows 256 -> 512 on the
    way); M = 1, 2 and the small clouds at extent 2.2 need every point, so the cap is given as M there, elsewhere it is
    the default M / 2."""
    src = _factor_cloud(m, dim, scale)
    default_cap = m == 1500 or (scale < 1.0 and m >= 255)
    plan = _open_plan(src, 1, 0 if default_cap else m)
    try:
        rank = plan.nonrigid_rank()
        fft = _product_with_kernel(plan)
    finally:
        plan.close()
    g = ob.kernel(ob.plan_coords(src, centre=False))
    err = float(np.max(np.abs(g - fft)))
    print("BCPD_LOWRANK factor m=%d dim=%d scale=%g rank=%d max|G-FF^T|=%.2e" % (m, dim, scale, rank, err))
    assert 1 <= rank <= m
    assert err <= KERNEL_TOL
    if m == 1500 and dim == 3 and scale == 1.0:
        assert 256 < rank < 750
    if scale < 1.0 and m >= 255:
        assert rank < 100


def test_duplicated_points_are_never_a_second_pivot():
    """237 distinct points at an extent of 22 (their kernel matrix has full numerical rank) and 20 copies: once a point is a
    pivot the remaining diagonal entry of its copy is round-off, far below tol, so the rank is the number of DISTINCT
    points - one more would be a copy, and a column divided by the square root of round-off."""
    from probreg_amd import synthetic

    base = synthetic.surface(237, 5) * 10.0
    src = np.concatenate([base, base[7:27]], axis=0)[np.random.default_rng(5).permutation(257)]
    y = ob.plan_coords(src, centre=False)
    assert np.unique(y, axis=0).shape[0] == 237
    assert ob.pivoted_cholesky(y, KERNEL_TOL, 257).f.shape[1] == 237
    plan = _open_plan(src, 1, 257)
    try:
        rank = plan.nonrigid_rank()
        fft = _product_with_kernel(plan)
    finally:
        plan.close()
    err = float(np.max(np.abs(ob.kernel(y) - fft)))
    print("BCPD_LOWRANK duplicates rank=%d max|G-FF^T|=%.2e" % (rank, err))
    assert rank == 237
    assert np.all(np.isfinite(fft)) and err <= KERNEL_TOL


# ---- a kernel that is not low rank ----------------------------------------------------------------------------------------
def _wide_cloud():
    from probreg_amd import synthetic

    return synthetic.surface(1500, 9) * 10.0


def test_lowrank_refuses_a_cloud_that_is_not_low_rank():
    with pytest.raises(ValueError, match=r"rank 750\b.*G - F F\^T is still") as info:
        _open_plan(_wide_cloud(), 1).close()
    print("BCPD_LOWRANK refusal: %s" % info.value)


def test_auto_keeps_the_dense_matrix_where_the_factor_does_not_converge():
    """... and then solves as tests/test_bcpd_gpu.py::test_solve_matches_dense_inverse asks of a dense plan."""
    from oracle import bcpd_numpy as bo
    from probreg_amd import bcpd
    from conftest import rel_err

    src = _wide_cloud()
    rng = np.random.default_rng(7)
    m = src.shape[0]
    nu = rng.uniform(0.0, 2.0, m)
    nu[rng.choice(m, 60, replace=False)] = 0.0
    resid = rng.normal(0.0, 0.3, (m, 3))
    lmd, cfac = 2.0, 37.5
    plan = _open_plan(src, 2)
    try:
        assert plan.nonrigid_rank() == 0
        v, sd = plan.bcpd_solve(lmd, cfac, resid, nu)
    finally:
        plan.close()
    g = bo.inverse_multiquadric_kernel(src, src).astype(np.float64)
    sigma = np.linalg.inv(lmd * np.linalg.inv(g) + cfac * np.diag(nu))
    assert rel_err(sd, np.diag(sigma)) < 1e-6
    assert rel_err(v, cfac * sigma @ (nu[:, None] * resid)) < 1e-6
    reg = bcpd.CombinedBCPD(src, solver="auto")
    try:
        assert reg.kernel_rank == 0
    finally:
        reg._close_plan()


# ---- the M-step on the factor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ob.SOLVE_CASES, ids=ob.case_id)
def test_solve_on_the_factor(case):
    from probreg_amd import engine

    inp = ob.solve_inputs(case)
    max_rank, tol = ob.case_rank_and_tol(case)
    if case.shuffle:   # the plan sorts the cloud and pivots in ITS order: the restatement is run in the same one
        order = engine.spatial_order(inp.src)
        assert not np.array_equal(order, np.arange(case.m))
        ref = ob.reference_on(ob.plan_coords(inp.src, centre=False), case, inp, order=order)
    else:
        ref = ob.solve_reference(case)
    plan = _open_plan(inp.src, 1, max_rank, tol, sort_source=case.shuffle)
    try:
        rank = plan.nonrigid_rank()
        v, sd = plan.bcpd_solve(case.lmd, case.cfac, inp.resid, inp.nu)
    finally:
        plan.close()
    scale_v = max(float(np.max(np.abs(ref.v_dense))), 1e-300)
    rows = [("v_hat", ob.rel_max(v, ref.v), ob.bound(ref.y_v, case.m), float(np.max(np.abs(v - ref.v_dense))) / scale_v,
             ref.e_trunc_v, ref.y_v),
            ("diag_sigma", ob.rel_max(sd, ref.sd), ob.bound(ref.y_sd, case.m), ob.rel_max(sd, ref.sd_dense), ref.e_trunc_sd,
             ref.y_sd)]
    bad = []
    for q, err_lr, lim_lr, err_dense, e_trunc, y in rows:
        lim_dense = 4.0 * e_trunc + lim_lr
        print("BCPD_LOWRANK solve %s %s rank=%d(host %d) y=%.1e vs-lowrank=%.1e limit=%.1e | e_trunc=%.1e vs-dense=%.1e limit=%.1e"
              % (ob.case_id(case), q, rank, ref.rank, y, err_lr, lim_lr, e_trunc, err_dense, lim_dense))
        if not err_lr <= lim_lr:
            bad.append((q, "low-rank restatement", err_lr, lim_lr))
        if not err_dense <= lim_dense:
            bad.append((q, "dense form", err_dense, lim_dense))
    assert rank <= case.m and (case.max_rank is None or rank == case.max_rank)
    assert np.all(sd >= 0.0)
    if case.nu == "allzero":   # A = I: no pull at all, and Sigma = F F^T / lmd
        assert not np.any(v)
        assert ob.rel_max(sd, ref.ffT_diag / case.lmd) <= ob.bound(0.0, case.m)
    assert not bad, (ob.case_id(case), bad)


# ---- whole registrations --------------------------------------------------------------------------------------------------
REG_KW = dict(w=0.1, maxiter=10, tol=-1.0)


@pytest.fixture(scope="module")
def reg_pair():
    from probreg_amd import synthetic

    src, tgt = synthetic.nonrigid_pair(1500, 1400, seed=3)[:2]
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


@pytest.fixture(scope="module")
def reg_lowrank(reg_pair):
    from probreg_amd import bcpd

    src, tgt = reg_pair
    reg = bcpd.CombinedBCPD(src, solver="lowrank")
    try:
        rank = reg.kernel_rank
        trans = reg.registration(tgt, **REG_KW)
    finally:
        reg._close_plan()
    return rank, trans


def _same_bytes(a, b):
    return (np.array_equal(a.rigid_trans.rot, b.rigid_trans.rot) and np.array_equal(a.rigid_trans.t, b.rigid_trans.t)
            and a.rigid_trans.scale == b.rigid_trans.scale and np.array_equal(a.v, b.v))


def _compare_transformations(tag, trans, src, t_ref, rot_ref, scale_ref):
    from conftest import rel_err

    e_t, e_r, e_s = rel_err(trans.transform(src), t_ref), rel_err(trans.rigid_trans.rot, rot_ref), abs(trans.rigid_trans.scale - scale_ref)
    print("BCPD_LOWRANK registration %s T=%.2e rot=%.2e scale=%.2e (limit %.0e)" % (tag, e_t, e_r, e_s, TOL_T))
    assert e_t < TOL_T and e_r < TOL_T and e_s < TOL_T


def test_registration_matches_the_dense_form_on_the_host(reg_pair, reg_lowrank):
    src, tgt = reg_pair
    rank, trans = reg_lowrank
    assert 256 < rank < src.shape[0] // 2
    g = ob.kernel(ob.plan_coords(src))
    res = ob.registration(src, tgt, REG_KW["w"], REG_KW["maxiter"],
                          lambda nu, resid, lmd, cfac: ob.solve_dense(g, nu, resid, lmd, cfac))
    _compare_transformations("vs host dense form", trans, src, ob.transformed(res, src), res.rot, res.scale)


def test_registration_matches_the_dense_solver_on_the_device(reg_pair, reg_lowrank):
    from probreg_amd import bcpd

    src, tgt = reg_pair
    dense = bcpd.registration_bcpd(src, tgt, solver="dense", **REG_KW)
    _compare_transformations("vs device dense", reg_lowrank[1], src, dense.transform(src), dense.rigid_trans.rot,
                             dense.rigid_trans.scale)


def test_registration_is_byte_repeatable(reg_pair, reg_lowrank):
    from probreg_amd import bcpd

    src, tgt = reg_pair
    again = bcpd.registration_bcpd(src, tgt, solver="lowrank", **REG_KW)
    assert _same_bytes(again, reg_lowrank[1])


def test_default_solver_is_the_dense_one():
    from probreg_amd import bcpd, synthetic

    src, tgt = synthetic.nonrigid_pair(330, 300, seed=8)[:2]
    a = bcpd.registration_bcpd(src, tgt, w=0.1, maxiter=5, tol=-1.0)
    b = bcpd.registration_bcpd(src, tgt, w=0.1, maxiter=5, tol=-1.0, solver="dense")
    assert _same_bytes(a, b)
    reg = bcpd.CombinedBCPD(src)
    try:
        assert reg.solver == "dense" and reg.kernel_rank == 0
    finally:
        reg._close_plan()
    with pytest.raises(ValueError):
        bcpd.CombinedBCPD(src, solver="sparse")
