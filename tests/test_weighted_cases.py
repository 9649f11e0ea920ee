"""Preconditions of tests/test_weighted_estep_gpu.py, held with the fp64 oracles alone (no GPU): every case of
tests/weighted_cases.py leaves enough mass to compare, its weights stay inside what the float32 storage of ln a_m resolves and clear of
the clamp in bcpd._estep_on_plan, the dead columns and dead rows are exact zeros of the ORACLE, and the weights change the answer by
far more than any bound of the GPU file - so a failure there is never the case's own fault."""
import numpy as np
import pytest

import weighted_cases as wc

FULL = wc.grid_cases() + wc.two_d_cases() + wc.swapped_cases()   # the full-size cases on the default weights
TILES = wc.tile_cases()
DEAD, UNIFORM = wc.special_cases()


def test_sizes_and_weight_sets():
    for k in (wc.M_DEFAULT, wc.N_DEFAULT):
        assert all(k % q for q in (32, 128, 256, 512)) and k > 3 * 512
    assert len(FULL) == 12 + 3 + 4 and len(set(wc.all_cases())) == len(wc.all_cases())
    assert len(set(wc.case_id(c) for c in wc.all_cases())) == len(wc.all_cases())
    alpha, sd = wc.weights(wc.M_DEFAULT, 3, 0.01)
    again = wc.weights(wc.M_DEFAULT, 3, 0.01)
    assert np.array_equal(alpha, again[0]) and np.array_equal(sd, again[1])
    assert abs(alpha.sum() - 1.0) < 1e-12 and np.all(alpha > 0.0)
    ex = sd * 3 / (2.0 * 0.01)   # the exponent of exp(-s^2 D Sigma_mm / 2 sigma2) at scale 1
    assert ex.min() >= 0.0 and 11.0 < ex.max() <= 12.0
    # the outlier weight follows the families' rule
    assert [c.base.w for c in wc.grid_cases() if c.base.family == "lopsided"] == [0.1, 0.0, 0.0]
    assert all(c.base.w == 0.1 for c in wc.grid_cases() if c.base.family != "lopsided")
    # every near pose is a rigid map at scale 1: the exponent bound above is the cases'
    assert all(wc.case_setup(c)["st_c"].scale == 1.0 for c in wc.all_cases())
    a_u, sd_u = wc.case_weights(UNIFORM)
    assert np.all(a_u == 1.0 / wc.M_DEFAULT) and np.all(sd_u == 0.0)


@pytest.mark.parametrize("c", FULL + TILES, ids=wc.case_id)
def test_weights_stay_inside_float32_and_clear_of_the_clamp(c):
    """ln a_m - max is uploaded as float32 (relative 6e-8): a span <= 20 costs a term at most 1.2e-6 relative.  -max(ln a) < 700 keeps
    the min(-top, 700) clamp of bcpd._estep_on_plan out of the picture."""
    lw = wc.log_weights(c)
    print("%s: ln a spans %.2f, -max %.2f" % (wc.case_id(c), lw.max() - lw.min(), -lw.max()))
    assert np.all(np.isfinite(lw)) and lw.max() < 0.0
    assert lw.max() - lw.min() <= 20.0
    assert -lw.max() < 700.0


@pytest.mark.parametrize("c", FULL, ids=wc.case_id)
def test_no_full_size_case_is_degenerate(c):
    b = c.base
    es, plain = wc.oracle_estep(c), wc.oracle_plain(c)
    moved = float(np.max(np.abs(es.nu - plain.p1)))
    print("%s: sigma2 %.4e n_p/N %.4f max nu %.1f max |px| %.1f max |nu - p1 unweighted| %.2f" % (
        wc.case_id(c), wc.case_setup(c)["st_c"].sigma2, es.n_p / b.n, es.nu.max(), np.abs(es.px).max(), moved))
    assert all(np.all(np.isfinite(a)) for a in (es.nu_d, es.nu, es.px)) and np.isfinite(es.n_p)
    assert es.n_p >= 0.4 * b.n                       # (measured minimum: 0.412, aniso late)
    assert moved > 1.0                               # a kernel that ignored the weights fails every bound (measured: 2.7 .. 363)
    zero = np.flatnonzero(es.nu_d == 0.0)
    if b.family == "lopsided" and b.state == "late":
        # the blob without a partner: exactly those columns, exactly zero (the oracle's den == 0 rule, bcpd.py:64)
        assert b.w == 0.0 and b.n // 4 == 475
        assert np.array_equal(zero, np.arange(b.n // 4))
        assert abs(es.n_p - (b.n - zero.size)) < 1e-9 * b.n
    else:
        assert zero.size == 0
        if b.w == 0.0:
            assert abs(es.n_p - b.n) < 1e-9 * b.n    # every column of P sums to one


@pytest.mark.parametrize("c", TILES, ids=wc.case_id)
def test_tile_edge_cases(c):
    """A handful of points cannot hold every target against the uniform term (3 x 700 at w = 0.1: n_p = 0.14 N), so the mass bound of
    the full-size cases is not asked here; with w = 0 every column sums to one, which is what the GPU file holds the pads to."""
    b = c.base
    es, plain = wc.oracle_estep(c), wc.oracle_plain(c)
    print("%s: n_p/N %.4f max nu %.2f max |nu - p1 unweighted| %.3f" % (
        wc.case_id(c), es.n_p / b.n, es.nu.max(), np.max(np.abs(es.nu - plain.p1))))
    assert all(np.all(np.isfinite(a)) for a in (es.nu_d, es.nu, es.px))
    assert np.all(es.nu_d > 0.0) and es.n_p >= 0.1 * b.n
    if b.w == 0.0:
        assert abs(es.n_p - b.n) < 1e-9 * b.n and np.max(np.abs(es.nu_d - 1.0)) < 1e-9
    # the weights move nu by more than a thousand times the 2e-5 max(1, max nu) the GPU file allows
    assert np.max(np.abs(es.nu - plain.p1)) > 1e3 * 2e-5 * max(1.0, es.nu.max())


def test_dead_rows_are_exact_zeros_of_the_oracle():
    """An exponent of 2000: a_m underflows to exactly 0 in fp64, so nu and px of those rows are exact zeros; the rest of the case is
    as healthy as `clusters mid` itself."""
    es = wc.oracle_estep(DEAD)
    dead = wc.dead_rows(DEAD.base.m)
    assert dead.size == 300 and dead[1] == 7
    assert np.all(es.nu[dead] == 0.0) and np.all(es.px[dead] == 0.0)
    alive = np.delete(np.arange(DEAD.base.m), dead)
    assert np.all(es.nu[alive] > 0.0)
    assert es.n_p >= 0.4 * DEAD.base.n and np.all(es.nu_d > 0.0)
    lw = wc.log_weights(DEAD)
    assert -lw.max() < 700.0 and np.all(lw[dead] - lw.max() < -1900.0)
    assert np.max(np.abs(es.nu - wc.oracle_plain(DEAD).p1)) > 1.0


def test_uniform_weights_are_the_plain_estep():
    """alpha = 1 / M, Sigma = 0: the weighted oracle (numpy) and the plain CPD oracle (C) compute the same E-step - the two
    references the GPU file uses agree far inside its bounds."""
    es, plain = wc.oracle_estep(UNIFORM), wc.oracle_plain(UNIFORM)
    assert np.max(np.abs(es.nu_d - plain.pt1)) < 1e-10
    assert np.max(np.abs(es.nu - plain.p1)) < 1e-10 * max(1.0, plain.p1.max())
    assert np.max(np.abs(es.px - plain.px)) < 1e-10 * max(1.0, np.abs(plain.px).max())
    assert abs(es.n_p - plain.n_p) < 1e-10 * plain.n_p
