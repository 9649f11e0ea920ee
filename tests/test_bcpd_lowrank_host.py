"""The NumPy restatement of BCPD on a low-rank kernel factor (tests/oracle_bcpd_lowrank.py) against its own dense form, on
the CPU: what the truncation G ~ F F^T costs, per solve case of tests/test_bcpd_lowrank_gpu.py.  No GPU, no product code
beyond the synthetic clouds.

Every case prints its rank, the yardstick y and the truncation error e_trunc (BCPD_LOWRANK_HOST lines); the GPU tests hold
the device to 4 * e_trunc against the dense form.

Truncation matters once cfac * nu * tol approaches lmd: the factor leaves up to tol in every entry of G, and Sigma sees it
multiplied by about cfac nu / lmd.  Taken here (surface clouds, nu uniform in [0, 2) with 8 % zeros, c = 1):
  surface(3000), lmd 2, cfac 1e3, tol 1e-11 (rank 519)   v_hat off by 2.8e-9 absolute on a max |v_hat| of 0.055, diag Sigma by
                                                         9.6e-9 of its maximum
  surface(1500), lmd 2, cfac 1e6, tol 1e-6  (rank 178)   v_hat off by 0.24 of its maximum, diag Sigma by 0.094: not usable.
                                                         (With other draws of nu the same set-up loses half of diag Sigma.)
so `kernel_tol` must stay small against lmd / (cfac nu); the default 1e-11 does for every cfac a registration reaches before
the float32 E-step stops resolving sigma2.
"""
import numpy as np
import pytest

import oracle_bcpd_lowrank as ob

KERNEL_TOL = 1e-11
NU_TYPICAL = 2.0
# e_trunc <= 100 (1 + cfac nu / lmd) tol: first order in E = G - F F^T, whose entries are <= tol and whose 2-norm is
# <= trace E <= M tol; d Sigma = lmd (lmd I + c G D)^-1 E (lmd I + c D G)^-1 acts on it with factors of size <= 1 where nu > 0 and
# passes it on as E / lmd where nu = 0, and v_hat = c Sigma D R multiplies by c nu / lmd once more.  100 stands for the
# dependence on M and the cloud (largest measured: 27 at m1500-lmd50-cfac1e5); a guard against gross error, not a fit.
TRUNC_CONSTANT = 100.0


@pytest.mark.parametrize("case", ob.SOLVE_CASES + [ob.GUARD_CASE], ids=ob.case_id)
def test_lowrank_solve_against_the_dense_form(case):
    inp = ob.solve_inputs(case)
    ref = ob.solve_reference(case)
    max_rank, tol = ob.case_rank_and_tol(case)
    print("BCPD_LOWRANK_HOST %s rank=%d resid=%.2e tol=%.2e y_v=%.1e y_sd=%.1e (solver alone %.1e %.1e) e_trunc_v=%.1e e_trunc_sd=%.1e"
          % (ob.case_id(case), ref.rank, ref.resid, tol, ref.y_v, ref.y_sd, ref.y_v_solver, ref.y_sd_solver, ref.e_trunc_v,
             ref.e_trunc_sd))
    assert ref.resid <= tol                                  # the factor converged ...
    if case.max_rank is not None:
        assert ref.rank == case.max_rank                     # ... a forced one at exactly its rank
    else:
        assert ref.rank < (max_rank or case.m // 2) or ref.rank == case.m
    assert np.all(ref.sd >= 0.0) and np.all(ref.sd_dense > 0.0)
    # the yardstick is round-off, far below anything it is used to judge
    assert ref.y_v <= 1e-8 and ref.y_sd <= 1e-8
    if case.nu == "allzero":
        assert not np.any(ref.v) and not np.any(ref.v_dense)
        assert ob.rel_max(ref.sd, ref.ffT_diag / case.lmd) <= 8 * case.m * 2.0 ** -53
        assert ref.e_trunc_sd <= tol / np.max(ref.sd_dense) / case.lmd * 1.0001   # Sigma = G / lmd: off by diag(E) / lmd
    if case.max_rank is None:
        limit = TRUNC_CONSTANT * (1.0 + case.cfac * NU_TYPICAL / case.lmd) * tol
        assert ref.e_trunc_v <= limit and ref.e_trunc_sd <= limit
    else:   # a rank of 1, 37 or 130 is nowhere near the kernel: these cases exercise tails, not accuracy
        assert ref.e_trunc_sd > 1e-4


def test_guard_figures():
    """The figures of the module docstring, within a factor of 4 either way."""
    ref = ob.solve_reference(ob.GUARD_CASE)
    abs_v = ref.e_trunc_v * float(np.max(np.abs(ref.v_dense)))
    print("BCPD_LOWRANK_HOST guard: |v_hat| max %.3g, off by %.2e absolute; diag Sigma off by %.2e of its maximum"
          % (float(np.max(np.abs(ref.v_dense))), abs_v, ref.e_trunc_sd))
    assert 2.8e-9 / 4 <= abs_v <= 2.8e-9 * 4
    assert 9.6e-9 / 4 <= ref.e_trunc_sd <= 9.6e-9 * 4
    loose = ob.solve_reference(ob.LOOSE_CASE)
    print("BCPD_LOWRANK_HOST loose tol: rank %d, v_hat off by %.2e, diag Sigma by %.2e" % (loose.rank, loose.e_trunc_v, loose.e_trunc_sd))
    assert loose.e_trunc_sd > 0.02 and loose.e_trunc_v > 0.05


def test_pivoted_cholesky_bounds_every_entry_and_skips_copies():
    from probreg_amd import synthetic

    base = synthetic.surface(237, 5) * 10.0
    src = np.concatenate([base, base[7:27]], axis=0)[np.random.default_rng(5).permutation(257)]
    y = ob.plan_coords(src, centre=False)
    fac = ob.pivoted_cholesky(y, KERNEL_TOL, 257)
    assert fac.converged and fac.pivots[0] == 0              # all diagonal entries tie at the start: lowest index
    assert np.max(np.abs(ob.kernel(y) - fac.f @ fac.f.T)) <= KERNEL_TOL
    picked = y[fac.pivots]
    assert np.unique(picked, axis=0).shape[0] == fac.pivots.size == 237   # never a copy of an earlier pivot
    # a cloud ten times the coherence length has no low-rank kernel: 0.037 left at rank 750
    wide = ob.pivoted_cholesky(ob.plan_coords(synthetic.surface(1500, 9) * 10.0, centre=False), KERNEL_TOL, 750)
    assert not wide.converged and wide.resid > 1e-3


def test_em_loop_on_the_factor_follows_the_dense_form():
    """Ten iterations on the 900-point version of the GPU test's pair: the truncation moves T by 2.7e-10."""
    from probreg_amd import synthetic

    src, tgt = synthetic.nonrigid_pair(900, 840, seed=3)[:2]
    y = ob.plan_coords(src)
    fac = ob.pivoted_cholesky(y, KERNEL_TOL, src.shape[0])   # (rank ~480: above the default cap of 840 / 2)
    assert fac.converged
    g = ob.kernel(y)
    dense = ob.registration(src, tgt, 0.1, 10, lambda nu, r, lmd, c: ob.solve_dense(g, nu, r, lmd, c))
    lowrank = ob.registration(src, tgt, 0.1, 10, lambda nu, r, lmd, c: ob.solve_lowrank(fac.f, nu, r, lmd, c))
    err = ob.rel_max(ob.transformed(lowrank, src), ob.transformed(dense, src))
    print("BCPD_LOWRANK_HOST EM loop: rank %d, T moved by %.2e after 10 iterations" % (fac.f.shape[1], err))
    assert err <= 1e-8
    assert np.max(np.abs(lowrank.rot - dense.rot)) <= 1e-8 and abs(lowrank.scale - dense.scale) <= 1e-8
