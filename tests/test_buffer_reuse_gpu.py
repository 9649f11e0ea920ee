"""Handles that are used again: one ``Permutohedral`` re-initialised across feature dimensions and sizes, one FilterReg plan
whose clouds are replaced.  Which device buffers such a handle keeps, re-creates or re-initialises (csrc/lattice.hip
lat_build, csrc/filterreg.hip prg_fr_set_source / prg_fr_set_target) must not show in any output: everything is compared,
bit for bit, with a FRESH handle given the same input, in the default splat mode (1: order-independent fixed-point sums)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("blur", [True, False])
def test_permutohedral_reinitialised_across_table_formats_and_sizes(blur):
    """d = 3 -> d = 5 -> d = 3 crosses the hash table's two entry formats ((generation << 48) | key for d <= 3, 64-bit
    hashes in a 0xFF-filled table for d > 3) both ways; the third lattice is smaller than the first, so only the change of d
    makes the tables new; the fourth is larger than any before."""
    from probreg_amd import gaussian_filtering as gf

    rng = np.random.default_rng(11)
    reused = None
    for d, n in ((3, 6000), (5, 3000), (3, 2000), (3, 9000)):
        pts = (rng.uniform(0.0, 1.0, (n, d)) * 6.0).astype(np.float32)
        vals = rng.normal(size=(n, 3)).astype(np.float32)
        if reused is None:
            reused = gf.Permutohedral(pts, blur)
        else:
            reused.init(pts, blur)
        fresh = gf.Permutohedral(pts, blur)
        assert reused.get_lattice_size() == fresh.get_lattice_size(), (d, n)
        for ch in (3, 1):
            got, want = reused.filter(vals[:, :ch]), fresh.filter(vals[:, :ch])
            assert np.any(want), (d, n, ch)
            assert np.array_equal(got, want), (d, n, ch, float(np.max(np.abs(got - want))))


def _clouds(rng, m, n):
    src = rng.normal(size=(m, 3))
    c, s = np.cos(0.2), np.sin(0.2)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    tgt = src[rng.integers(0, m, n)] @ rot.T + np.array([0.1, -0.05, 0.02]) + 0.01 * rng.normal(size=(n, 3))
    return src, tgt


def _em_step(plan):
    plan.set_state(np.identity(3), np.zeros(3), 0.05)
    size, blur = plan.estep()
    out = plan.mstep(0.1, True, "pt2pt", 1.0e-4)
    m0, m1, m2 = plan.get_estep(True)
    return size, blur, out, plan.get_state(), m0, m1, m2


def test_filterreg_plan_with_replaced_clouds_equals_a_fresh_plan():
    from probreg_amd import filterreg

    rng = np.random.default_rng(12)
    src_a, tgt_a = _clouds(rng, 5000, 5000)
    src_b, tgt_b = _clouds(rng, 7000, 3000)
    reused = filterreg._Plan()
    reused.set_source(src_a)
    reused.set_target(tgt_a)
    first = _em_step(reused)
    assert first[3][16] == 1.0 and np.isfinite(first[3]).all()  # (the first pair was really fitted)
    reused.set_target(tgt_b)  # smaller than before
    reused.set_source(src_b)  # larger than before
    got = _em_step(reused)
    fresh = filterreg._Plan()
    fresh.set_source(src_b)
    fresh.set_target(tgt_b)
    want = _em_step(fresh)
    assert want[3][16] == 1.0 and np.isfinite(want[3]).all()
    assert got[:2] == want[:2]
    for g, w in zip(got[2:], want[2:]):
        assert np.array_equal(g, w)
    reused.close()
    fresh.close()
