"""Host checks of tests/oracle_helpers.py: each restatement against what the project already trusts (the oracles under oracle/
and the reference's own fixtures), and every condition tests/test_helpers_gpu.py relies on - the Gauss bounds are neither vacuous
nor too tight for a faithful evaluation, no rbf case has a fragile entry, the planted clouds are what they claim to be."""
import os

import numpy as np
import pytest

import oracle_helpers as oh
from conftest import GOLDEN_DIR, Golden
from oracle import bcpd_numpy as bo
from oracle import cpd_numpy as co
from oracle import gauss_numpy as go

LD = oh.LD
TINY64 = 1e-300  # the fixtures are fp64 evaluations: entries below the normal range have lost their digits, or are 0
GG = Golden(os.path.join(GOLDEN_DIR, "gauss_golden.npz"))
GAUSS_CASES = [(s, t, dim) for dim in (2, 3) for s, t in oh.GAUSS_SIZES]


def _ratio(got, want, bound):
    return float(np.max(np.abs(np.asarray(got).astype(LD) - want) / bound))


# ------------------------------------------------------------------------------------------------------------------ pins
@pytest.mark.parametrize("s,t,dim", [(5, 70, 2), (257, 70, 3), (70, 513, 3)])
def test_gauss_terms_vs_oracle(s, t, dim):
    src, tgt, _, h = oh.gauss_case(s, t, dim)
    w = oh.gauss_case(s, t, dim, rows=3)[2]
    for weights in (w[0], w):
        want, big_a, big_b = oh.gauss_terms(src, tgt, weights, h)
        got = go.compute(src, h, tgt, weights)
        assert got.shape == want.shape
        assert _ratio(got, want, oh.gauss_bound_f64(big_a, big_b, s)) <= 1.0


@pytest.mark.parametrize("name", GG.group("gt"))
def test_gauss_terms_vs_reference_fixture(name):
    """The reference's own fp64 outputs (first 300 targets of the 5000-point cases) to fp64 rounding: within the fp64 bound."""
    c = GG.case("gt/" + name)
    s = c["source"].shape[0]
    w = c.get("weights")
    w = np.ones(s) if w is None else w
    want, big_a, big_b = oh.gauss_terms(c["source"], c["target"][:300], w, c["h"])
    out = c["out"][..., :300]
    assert out.shape == want.shape
    assert _ratio(out, want, oh.gauss_bound_f64(big_a, big_b, s) + TINY64) <= 1.0


@pytest.mark.parametrize("name", GG.group("l2"))
def test_l2_terms_vs_reference_fixture(name):
    """Gradient rows of the first 300 components (a row depends on its own source component only); the value where the whole
    fixture is small."""
    c = GG.case("l2/" + name)
    k = c["mu_target"].shape[0]
    whole = c["mu_source"].shape[0] <= 1000
    n = c["mu_source"].shape[0] if whole else 300
    f, fb, g, gb = oh.l2_terms(c["mu_source"][:n], c["phi_source"][:n], c["mu_target"], c["phi_target"], c["sigma"],
                               lambda a, b: oh.gauss_bound_f64(a, b, k))
    assert np.all(np.abs(c["out_g"][:n].astype(LD) - g) <= gb + TINY64)
    if whole:
        assert abs(LD(c["out_f"]) - f) <= fb
    f2, g2 = go.compute_l2_dist(c["mu_source"][:n], c["phi_source"][:n], c["mu_target"], c["phi_target"], c["sigma"])
    assert abs(LD(f2) - f) <= fb and np.all(np.abs(g2.astype(LD) - g) <= gb + TINY64)


def test_sks_pairwise_vs_oracle(cpd_golden):
    m = cpd_golden.case("misc")
    want, u = oh.sks_pairwise(m["x15"], m["x15"])
    assert abs(float(want) - m["sks_x15"]) < 1e-5  # (the fixture is a float32 scalar of value ~37)
    assert abs(co.squared_kernel_sum_closed_form(m["x15"], m["x15"]) - float(want)) <= 1e-13 * float(u)
    c = cpd_golden.case("reg/bunny_rigid_default")
    want, u = oh.sks_pairwise(c["source"], c["target"])
    assert abs(float(want) - m["sks_bunny"]) < 1e-6 * m["sks_bunny"]
    assert abs(co.squared_kernel_sum_closed_form(c["source"], c["target"]) - float(want)) <= 1e-13 * float(u)
    for dim in (1, 4, 33):
        x, y = oh.grid_cloud(63, dim, 0), oh.grid_cloud(64, dim, 1)
        want, u = oh.sks_pairwise(x, y)
        assert u >= want > 0
        assert abs(co.squared_kernel_sum_closed_form(x, y) - float(want)) <= 1e-13 * float(u)


def test_rbf_f32_vs_oracle(cpd_golden):
    m = cpd_golden.case("misc")
    k, _ = oh.rbf_f32(m["x15"] * 0.1, m["x15"] * 0.1, 1.0)
    assert np.max(np.abs(k - m["rbf_x15_beta1"])) < 2e-7
    c = cpd_golden.case("reg/fish_rigid_default")
    k, _ = oh.rbf_f32(c["source"], c["source"], 2.0)
    assert np.max(np.abs(k - m["rbf_fish_beta2"])) < 2e-7
    for dim in (2, 3):
        x, y = oh.kernel_case(33, 257, dim)
        for beta in oh.RBF_BETAS:
            k, _ = oh.rbf_f32(x, y, beta)
            ref = co.rbf_kernel(x, y, beta)
            # the oracle takes the exponential in float32 (and sums the squares through einsum): a float32 ulp or two
            assert k.dtype == np.float32 and np.max(np.abs(k - ref)) <= 2.0 ** -22


def test_imq_f32_vs_oracle():
    for dim in (2, 3):
        x, y = oh.kernel_case(33, 257, dim)
        for c in oh.IMQ_CS:
            assert np.array_equal(oh.imq_f32(x, y, c), bo.inverse_multiquadric_kernel(x, y, c))


def test_nn_mean_vs_kdtree():
    from scipy.spatial import cKDTree

    src, tgt = oh.rmse_case(70, 513, 3)
    want = np.mean(cKDTree(tgt).query(src)[0])
    assert abs(oh.nn_mean(src, tgt) - want) <= oh.RMSE_TOL * want
    assert abs(oh.nn_mean(src + 1e6, tgt + 1e6) - want) <= 1e-6 * want


# ------------------------------------------------------------------------------------------- what the GPU file relies on
@pytest.mark.parametrize("s,t,dim", GAUSS_CASES)
def test_gauss_bounds_are_neither_vacuous_nor_tight(s, t, dim):
    src, tgt, w, h = oh.gauss_case(s, t, dim)
    want, big_a, big_b = oh.gauss_terms(src, tgt, w, h)
    b32 = oh.gauss_bound_f32(big_a, big_b, np.sum(np.abs(w)))
    b64 = oh.gauss_bound_f64(big_a, big_b, s)
    d = tgt[:, None, :] - src[None, :, :]
    a = np.sum(d * d, axis=2) / h ** 2
    assert a.min() < 1.0 and (a.max() > 60.0 or t == 1)  # (one target has one distance range: t = 1 is the near one)
    # a faithful evaluation stays within HALF of each bound
    r32 = _ratio(oh.gauss_emulate_f32(src, tgt, w, h), want, b32)
    r64 = _ratio(oh.gauss_plain_f64(src, tgt, w, h), want, b64)
    print("gauss s=%d t=%d dim=%d: emulation err/bound fp32 %.3f fp64 %.3f" % (s, t, dim, r32, r64))
    assert r32 <= 0.5 and r64 <= 0.5
    # ... and a wrong one does not: the last source point dropped (its weight zeroed), h off by 1e-5
    w_drop = w.copy()
    w_drop[-1] = 0.0
    for wrong_w, wrong_h in ((w_drop, h), (w, h * (1.0 + 1e-5))):
        assert _ratio(oh.gauss_emulate_f32(src, tgt, wrong_w, wrong_h), want, b32) > 1.0
        assert _ratio(oh.gauss_plain_f64(src, tgt, wrong_w, wrong_h), want, b64) > 1.0


@pytest.mark.parametrize("rows", oh.GAUSS_ROWS)
def test_gauss_row_cases_within_half_bound(rows):
    src, tgt, w, h = oh.gauss_case(257, 70, 3, rows=rows)
    w2 = np.atleast_2d(w)
    assert np.any(w2 < 0) and np.any(w2 > 0)
    want, big_a, big_b = oh.gauss_terms(src, tgt, w2, h)
    b32 = oh.gauss_bound_f32(big_a, big_b, np.sum(np.abs(w2), axis=1)[:, None])
    assert _ratio(oh.gauss_emulate_f32(src, tgt, w2, h), want, b32) <= 0.5
    assert _ratio(oh.gauss_plain_f64(src, tgt, w2, h), want, oh.gauss_bound_f64(big_a, big_b, 257)) <= 0.5


@pytest.mark.parametrize("k", oh.L2_SIZES)
@pytest.mark.parametrize("dim", [2, 3])
def test_l2_cases_within_half_bound(k, dim):
    args = oh.l2_case(k, dim)
    f, fb, g, gb = oh.l2_terms(*args, bound=lambda a, b: oh.gauss_bound_f64(a, b, k))
    f2, g2 = go.compute_l2_dist(*args)
    assert fb > 0 and np.all(gb > 0)
    assert abs(LD(f2) - f) <= 0.5 * fb and np.all(np.abs(g2.astype(LD) - g) <= 0.5 * gb)
    # a value that is off by 1e-12 relative is outside the bound
    assert abs(f) * 1e-12 > fb


def test_rbf_cases_have_no_fragile_entry():
    """The GPU comparison is exact on every entry: none may sit on a float32 rounding boundary of the exponential."""
    count = 0
    for dim in (2, 3):
        for beta in oh.RBF_BETAS:
            xs = oh.kernel_square_case(dim)
            k, fragile = oh.rbf_f32(xs, xs, beta)
            assert not fragile.any()
            count += k.size
            for m in oh.KERNEL_M:
                for n in oh.KERNEL_N:
                    x, y = oh.kernel_case(m, n, dim)
                    k, fragile = oh.rbf_f32(x, y, beta)
                    assert not fragile.any(), (m, n, dim, beta, int(fragile.sum()))
                    count += k.size
    assert count > 500000
    # the mask itself, on values placed beside a float32 midpoint
    lo = np.float64(np.float32(0.7))
    mid = 0.5 * (lo + np.float64(np.nextafter(np.float32(0.7), np.float32(1))))
    v = np.array([mid * (1 + 2.0 ** -50), mid * (1 - 2.0 ** -50), mid * (1 + 2.0 ** -40), lo, 0.0])
    assert list(oh.round_f32_fragile(v)[1]) == [True, True, False, False, False]


def test_grid_clouds_are_float32_exact():
    for dim in oh.SKS_DIMS:
        x, y = oh.grid_cloud(257, dim, 0), oh.grid_cloud(255, dim, 1)
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
        d = x - y[0]
        assert np.array_equal(d.astype(np.float32).astype(np.float64), d)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("where", [0, 207, 208, 1024])
def test_planted_case_is_what_it_claims(dim, where):
    from scipy.spatial import cKDTree

    nseg, seg_len = oh.nn_segments(oh.PLANT_M, oh.PLANT_N)
    assert (nseg, seg_len) == (5, 208) and nseg * seg_len > oh.PLANT_N  # 0: first of the first; 207 | 208: an edge; 1024: last
    src, tgt, want = oh.planted_case(dim, where)
    assert src.shape == (oh.PLANT_M, dim) and tgt.shape == (oh.PLANT_N, dim)
    assert np.all(tgt.mean(axis=0) == 0.0) and np.all(tgt[where] == 0.0)
    dist, idx = cKDTree(tgt).query(src)
    assert np.all(idx == where)
    assert np.mean(dist) == want == oh.nn_mean(src, tgt)
    assert len({tuple(p) for p in src}) == oh.PLANT_M


def test_unshifted_closed_form_on_record():
    """The closed form on un-shifted float32 coordinates, as ``squared_kernel_sum`` evaluated it before it centred its clouds,
    beside the pairwise value of the fp64 inputs: printed for the log, and it must be what the far-offset GPU cases can see."""
    worst = {}
    for name, off in oh.SKS_FAR_OFFSETS.items():
        for m, n in oh.SKS_FAR_SHAPES[:1]:
            x, y = oh.far_pair(m, n, 3, off)
            want = float(oh.sks_pairwise(x, y)[0])
            got = oh.sks_unshifted_f64(x, y)
            worst[name] = abs(got - want) / want
            print("sks far %-6s %dx%d: pairwise %.12e  un-shifted float32 closed form %.12e  rel %.2e"
                  % (name, m, n, want, got, worst[name]))
    assert worst["1e6"] > 1e-6  # the bound of the GPU test separates the two formulations
