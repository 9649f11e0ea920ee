"""Preconditions of tests/test_estep_families_gpu.py, held with the fp64 oracle alone (no GPU): the cloud families of
tests/cloud_families.py are what they claim to be, and no case the GPU file runs is degenerate - enough mass left to compare
(n_p >= 0.7 N), nothing on the edge of fp64's underflow (where the oracle's own column sums would be a matter of rounding), the
matrix-core states inside the amplification the lean row pass and the fused sweep are specified for."""
import numpy as np
import pytest

import cloud_families as cf

ALL = cf.all_cases()


def _min_exponent(c):
    """min_m |x_n - z_m|^2 / (2 sigma2) per target column, from a kd-tree of the transformed source."""
    from scipy.spatial import cKDTree

    s = cf.case_setup(c)
    d, _ = cKDTree(cf.transformed(s["st"], s["src"])).query(s["tgt"])
    return d * d / (2.0 * s["st"].sigma2)


def test_generators_are_deterministic_float32_and_shaped():
    for family in cf.FAMILIES:
        src, tgt = cf.make_clouds(family)
        again = cf.make_clouds(family)
        assert src.shape == (cf.M_DEFAULT, 3) and tgt.shape == (cf.N_DEFAULT, 3)
        assert np.array_equal(src, again[0]) and np.array_equal(tgt, again[1])
        assert np.array_equal(src, src.astype(np.float32)) and np.array_equal(tgt, tgt.astype(np.float32))
        s2, t2 = cf.make_clouds(family, dim=2)
        assert np.array_equal(s2, src[:, :2]) and np.array_equal(t2, tgt[:, :2])
        sf, tf = cf.make_clouds(family, far=cf.FAR)
        assert np.max(np.abs(sf - src - np.array(cf.FAR))) < 1e-4 and np.max(np.abs(tf - tgt - np.array(cf.FAR))) < 1e-4
        # the swapped pair draws the same base sample: its source starts with the default source
        ss, ts = cf.make_clouds(family, m=cf.N_DEFAULT, n=cf.M_DEFAULT)
        assert ss.shape[0] == cf.N_DEFAULT and ts.shape[0] == cf.M_DEFAULT and np.array_equal(ss[:cf.M_DEFAULT], src)
    for k in (cf.M_DEFAULT, cf.N_DEFAULT):   # every last group, block and chunk is partly padded; the matrix cores are legal
        assert k >= 8192 and all(k % q for q in (32, 128, 256, 1024))
    # the shapes: a unit cube, a 10 : 1 : 1 box, two blobs 6 units apart, and a target blob the source lacks
    assert np.allclose(np.ptp(cf.make_clouds("volume")[0], axis=0), 1.0, atol=1e-2)
    assert np.allclose(np.ptp(cf.make_clouds("aniso")[0], axis=0), [10.0, 1.0, 1.0], atol=1e-2)
    src, tgt = cf.make_clouds("clusters")
    assert abs(np.mean(src[:, 0] > 3.0) - 0.5) < 0.02 and not np.any((src[:, 0] > 2.5) & (src[:, 0] < 4.5))
    src, tgt = cf.make_clouds("lopsided")
    dead = cf.dead_columns("lopsided", tgt.shape[0])
    assert dead.size == 2250 and src[:, 0].max() < 2.5 and np.all(tgt[dead, 0] > 5.0)
    assert np.array_equal(np.flatnonzero(tgt[:, 0] > 3.0), dead)


def test_poses_and_states():
    src, tgt = cf.make_clouds("clusters")
    for name, affine in (("near", False), ("jump", False), ("near", True)):
        lin, t, scale = cf.pose(src, tgt, name, affine)
        assert np.allclose(scale * lin @ src.mean(0) + t, tgt.mean(0), atol=1e-12)
        assert np.allclose(lin.T @ lin, np.eye(3), atol=1e-12) != affine
    lin2, _, _ = cf.pose(src[:, :2], tgt[:, :2])
    assert lin2.shape == (2, 2) and np.allclose(lin2.T @ lin2, np.eye(2), atol=1e-12)
    # the same map in the centred frame
    st = cf.make_state("clusters", "mid", src, tgt)
    s32, t32, cy, cx = cf.centred(src, tgt)
    assert s32.dtype == np.float32 and t32.dtype == np.float32
    assert np.allclose(cf.transformed(cf.centred_state(st, cy, cx), src - cy) + cx, cf.transformed(st, src), atol=1e-12)
    dense = cf.sigma2_of("clusters", "dense", src, tgt)
    assert st.sigma2 == 0.02 * dense and cf.sigma2_of("clusters", "jump", src, tgt) == st.sigma2 / 50.0
    assert cf.sigma2_of("clusters", "late", src, tgt) == 4e-4 and cf.sigma2_of("lopsided", "late", src, tgt) == 2e-3


@pytest.mark.parametrize("c", ALL, ids=cf.case_id)
def test_no_case_of_the_gpu_file_is_degenerate(c):
    s = cf.case_setup(c)
    es = cf.oracle_estep(c)
    amp = cf.amplification(s["tgt"], s["st"].sigma2)
    print("%s: sigma2 %.4e n_p/N %.4f amplification %.1f max p1 %.1f max |px| %.1f" % (
        cf.case_id(c), s["st"].sigma2, es.n_p / c.n, amp, es.p1.max(), np.abs(es.px).max()))
    # every column and every row takes part in the comparisons: nothing to mask
    assert all(np.all(np.isfinite(a)) for a in (es.pt1, es.p1, es.px)) and np.isfinite(es.n_p)
    assert es.n_p >= 0.7 * c.n
    dead = cf.dead_columns(c.family, c.n)
    if c.w == 0.0 and not (c.family == "lopsided" and c.state == "late"):
        assert abs(es.n_p - c.n) < 1e-9 * c.n and np.all(es.pt1 > 0.0)   # every column of P sums to one
    if c.family == "lopsided" and c.state == "late":
        # the blob without a partner is dead - exactly those columns, exactly zero - and three quarters of the mass are left
        assert c.w == 0.0
        assert np.array_equal(np.flatnonzero(es.pt1 == 0.0), dead) and dead.size == c.n // 4 == 2250
        assert abs(es.n_p - (c.n - dead.size)) < 1e-9 * c.n
    # no column near fp64's underflow edge (exp(-745) is the last denormal): there the oracle's den == 0 rule would turn on rounding
    ex = _min_exponent(c)
    assert not np.any((ex > 700.0) & (ex < 760.0)), float(np.min(np.abs(ex - 730.0)))
    if dead.size and c.state == "late":
        assert np.all(ex[dead] > 760.0) and np.all(np.delete(ex, dead) < 700.0)
    if c.state == "jump_deep":   # what makes the case lean on the motion bound: columns beyond 2^-48 of the new sigma2 alone
        assert np.sum(ex > 48.0 * np.log(2.0)) > 0.05 * c.n
    # states the matrix-core engines run: inside the lean row pass' and the fused sweep's default amplification
    if c.state == "dense":
        assert amp <= 1.0
    elif c.state == "mid":
        assert 16.0 <= amp <= 64.0
    elif c.state == "late" and c.family in ("aniso", "clusters"):
        assert amp > 5000.0


def test_uniform_term_leaves_most_of_the_mass():
    """w = 0.1: at least 0.91 N left in every state of the three families whose target has a partner everywhere."""
    for c in cf.grid_cases():
        if c.w > 0.0 and c.family != "lopsided":
            assert cf.oracle_estep(c).n_p >= 0.91 * c.n, cf.case_id(c)


def test_why_lopsided_late_is_run_at_2e_3_and_w0_only():
    """At sigma2 = 4e-4 (the other families' late state) the blob without a partner is no clean case: with w = 0.1 less than a
    tenth of the mass is left, and columns sit in fp64's underflow band."""
    from oracle import cpd_c

    c = cf.case("lopsided", "late", 0.0)
    s = cf.case_setup(c)
    z, x = cf.transformed(s["st_c"], s["s32"].astype(np.float64)), s["t32"].astype(np.float64)
    _, _, _, n_p = cpd_c.expectation_step(z, x, 4e-4, 0.1)
    assert n_p < 0.7 * c.n
    ex = _min_exponent(c) * (s["st"].sigma2 / 4e-4)
    assert np.any((ex > 700.0) & (ex < 760.0))
