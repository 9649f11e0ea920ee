"""The stand-alone entry points of csrc/misc.hip (probreg_amd.math_utils, gauss_transform, cost_functions) at their launch edges,
against the restatements of tests/oracle_helpers.py: sizes on both sides of every pad, tile, workgroup cap and segment, every
entry within a derived bound (never a maximum over the output), bit equality where every operation is correctly rounded.  The
comparisons rest on tests/test_oracle_helpers.py: a faithful evaluation stays within half of each Gauss bound and a wrong one
leaves it, no rbf case has a fragile entry, the planted clouds are what they claim.

Measured on one MI355X, as worst |err| / bound over every entry of every case (bound 1): Gauss sizes 0.39 (fp32) and 0.46 (fp64),
weight rows 0.31 and 0.18, compute_l2_dist 0.037 (value) and 0.041 (gradient); squared_kernel_sum 4.8e-16 of the un-cancelled
magnitude U near the origin and above the workgroup caps (bound 1e-12), at most 1.9e-16 relative on the far-offset pairs
(bound 1e-6); compute_rmse 0.052 of its 2^-21; rbf_kernel and inverse_multiquadric_kernel equal on every entry.
Before squared_kernel_sum centred its clouds in fp64 (it cast the raw coordinates to float32) the far-offset pairs read, as
relative error at 700 x 900 / 5000 x 3000: offset (0, 0, 1277) 1.65e-6 / 8.7e-7, 1e4 7.0e-5 / 2.5e-5, 1e5 3.5e-5 / 8.4e-5,
1e6 2.0e-3 / 6.8e-3, the 33-dimensional pair at 1e4 7.3e-6, and FilterReg's first sigma2 moved by 1.3e-4 with clouds at +1e5.
Before prg_gauss_transform_direct kept its exponent scale finite, h = 1e-20 gave NaN on every coincident pair.
"""
import numpy as np
import pytest

import oracle_helpers as oh

pytestmark = pytest.mark.gpu

LD = oh.LD
GAUSS_CASES = [(s, t, dim) for dim in (2, 3) for s, t in oh.GAUSS_SIZES]


def _ratio(got, want, bound):
    return float(np.max(np.abs(np.asarray(got).astype(LD) - want) / bound))


def _bounds(src, tgt, w, h):
    want, big_a, big_b = oh.gauss_terms(src, tgt, w, h)
    sum_abs_w = np.sum(np.abs(w), axis=-1)
    b32 = oh.gauss_bound_f32(big_a, big_b, sum_abs_w[:, None] if np.ndim(w) == 2 else sum_abs_w)
    return want, {False: b32, True: oh.gauss_bound_f64(big_a, big_b, np.shape(src)[0])}


# ------------------------------------------------------------------------------------------------------------ Gauss transform
@pytest.mark.parametrize("s,t,dim", GAUSS_CASES)
def test_gauss_sizes_every_entry_within_bound(s, t, dim):
    """Sources of 1, 3, 4, 5 points (the walk of four) and 255, 256, 257 (the pad to 256); targets of 1 to 513 (lanes of the last
    workgroup without a target)."""
    from probreg_amd import gauss_transform as gt

    src, tgt, w, h = oh.gauss_case(s, t, dim)
    want, bound = _bounds(src, tgt, w, h)
    for exact in (False, True):
        got = gt.GaussTransform(src, h, exact=exact).compute(tgt, w)
        assert got.shape == (t,) and got.dtype == np.float64
        r = _ratio(got, want, bound[exact])
        print("gauss s=%d t=%d dim=%d exact=%s: worst |err| / bound %.3f" % (s, t, dim, exact, r))
        assert r <= 1.0, (exact, r)


@pytest.mark.parametrize("rows", oh.GAUSS_ROWS)
def test_gauss_weight_rows(rows):
    """1 to 9 rows: every grouping into sweeps of 4, 2 and 1 rows, 4 + 4 + 1 included.  Signed weights."""
    from probreg_amd import gauss_transform as gt

    src, tgt, w, h = oh.gauss_case(257, 70, 3, rows=rows)
    w = np.atleast_2d(w)
    want, bound = _bounds(src, tgt, w, h)
    for exact in (False, True):
        tr = gt.GaussTransform(src, h, exact=exact)
        got = tr.compute(tgt, w)
        assert got.shape == (rows, 70)
        r = _ratio(got, want, bound[exact])
        print("gauss rows=%d exact=%s: worst |err| / bound %.3f" % (rows, exact, r))
        assert r <= 1.0, (exact, r)
        if exact:  # (test_gauss_gpu.py checks this for seven fp32 rows)
            for k in range(rows):
                assert np.array_equal(got[k], tr.compute(tgt, w[k])), k


@pytest.mark.parametrize("dim", [2, 3])
def test_gauss_special_targets(dim):
    from probreg_amd import gauss_transform as gt

    src, _, w, h = oh.gauss_case(257, 70, dim)
    # bit-equal to a source point | 4 units beyond the cloud: every term below 2^-150, nothing of it left in float32, but above
    # fp64's underflow | every term below fp64's underflow too (a > 745) | where the pads are
    beyond = np.zeros(dim)
    beyond[0] = src[:, 0].max() + 4.0
    tgt = np.stack([src[100], beyond, src[0] + 20.0, np.full(dim, 1e18)])
    d = tgt[:, None, :] - src[None, :, :]
    a = np.sum(d * d, axis=2) / h ** 2
    assert a[0].min() == 0.0 and 110.0 < a[1].min() < 700.0 and a[2].min() > 750.0
    want, bound = _bounds(src, tgt, w, h)
    got32 = gt.GaussTransform(src, h).compute(tgt, w)
    got64 = gt.GaussTransform(src, h, exact=True).compute(tgt, w)
    # (target 2 in fp64: the terms are below fp64's smallest number and the bound, a multiple of them, cannot be met by any
    # fp64 value but through them; the exact 0.0 asserted below is the check there)
    for got, b, rows in ((got32, bound[False], [0, 1, 2, 3]), (got64, bound[True], [0, 1, 3])):
        assert np.all(np.isfinite(got))
        err = np.abs(got.astype(LD) - want)
        assert np.all(err[rows] <= b[rows]), (err, b)
    assert got32[1] == 0.0 and got32[2] == 0.0 and got32[3] == 0.0
    assert got64[1] != 0.0 and got64[2] == 0.0 and got64[3] == 0.0


@pytest.mark.parametrize("k", oh.L2_SIZES)
@pytest.mark.parametrize("dim", [2, 3])
def test_compute_l2_dist_value_and_gradient_within_bound(k, dim):
    """K x K with 1 + dim weight rows (a sweep of two and one of one in 2-D, one sweep of four in 3-D), exponentials in fp64.
    The bound of the transform is carried through the host algebra as oracle_helpers.l2_terms states it."""
    from probreg_amd import cost_functions as cf

    args = oh.l2_case(k, dim)
    f, fb, g, gb = oh.l2_terms(*args, bound=lambda a, b: oh.gauss_bound_f64(a, b, k))
    got_f, got_g = cf.compute_l2_dist(*args, exact=True)
    assert got_g.shape == (k, dim)
    rf, rg = float(abs(LD(got_f) - f) / fb), _ratio(got_g, g, gb)
    print("l2 K=%d dim=%d: |err| / bound value %.3f gradient %.3f" % (k, dim, rf, rg))
    assert rf <= 1.0 and rg <= 1.0


def test_gauss_tiny_h_returns_the_weights():
    """h = 1e-20: exp(-0) = 1 on the coincident pair and 0 on every other.  (The fp32 entry formed kk = -inf and returned
    NaN = -inf x 0 here.)"""
    from probreg_amd import gauss_transform as gt

    src = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.5, 0.25, 3.0], [-1.5, -2.5, 0.5]])
    w = np.array([0.5, -1.25, 2.0, 3.5, -0.75])
    for dim in (2, 3):
        for exact in (False, True):
            got = gt.GaussTransform(src[:, :dim], 1e-20, exact=exact).compute(src[:, :dim], w)
            print("tiny h dim=%d exact=%s:" % (dim, exact), got)
            assert np.array_equal(got, w), (dim, exact, got)


# --------------------------------------------------------------------------------------------------------- squared_kernel_sum
@pytest.mark.parametrize("dim", oh.SKS_DIMS)
def test_sks_near_origin_shapes(dim):
    """dim 2 and 3 take the row-major kernels, every other the generic ones.  fp64 sums of at most a few hundred terms per lane
    plus a tree: 1e-12 of the un-cancelled magnitude leaves about 450 eps of margin."""
    from probreg_amd import math_utils as mu

    worst = 0.0
    for m, n in oh.SKS_SHAPES:
        x, y = oh.grid_cloud(m, dim, 0), oh.grid_cloud(n, dim, 1)
        want, u = oh.sks_pairwise(x, y)
        got = mu.squared_kernel_sum(x, y)
        worst = max(worst, float(abs(LD(got) - want) / u))
        assert abs(LD(got) - want) <= 1e-12 * u, (m, n, got, want)
    print("sks dim=%d: worst |err| / U %.2e" % (dim, worst))


def test_sks_dim_65_raises():
    from probreg_amd import math_utils as mu

    with pytest.raises(ValueError):
        mu.squared_kernel_sum(oh.grid_cloud(5, 65, 0), oh.grid_cloud(4, 65, 1))


@pytest.mark.parametrize("m,n,dim", oh.SKS_STRIDED)
def test_sks_above_the_workgroup_caps(m, n, dim):
    from probreg_amd import math_utils as mu

    x, y = oh.grid_cloud(m, dim, 0), oh.grid_cloud(n, dim, 1)
    want, u = oh.sks_pairwise(x, y)
    for got in (mu.squared_kernel_sum(x, y), mu.squared_kernel_sum(y, x)):
        print("sks %dx%d dim=%d: |err| / U %.2e" % (m, n, dim, float(abs(LD(got) - want) / u)))
        assert abs(LD(got) - want) <= 1e-12 * u


@pytest.mark.parametrize("dim", [3, 4])
def test_sks_exact_zeros(dim):
    from probreg_amd import math_utils as mu

    x, y = oh.grid_cloud(257, dim, 0), oh.grid_cloud(255, dim, 1)
    x[:, 1] = 0.0
    y[:, 1] = 0.0
    want, u = oh.sks_pairwise(x, y)
    assert abs(LD(mu.squared_kernel_sum(x, y)) - want) <= 1e-12 * u
    # a cloud against itself moved by v: the mean of |x_a - x_b - v|^2 over all pairs is 2 sum_a |x_a - mean|^2 / M + |v|^2
    v = np.array([0.5, -2.0, 0.25, 1.0][:dim])
    xl = x.astype(LD)
    closed = (2 * np.sum((xl - xl.mean(axis=0)) ** 2) / x.shape[0] + np.sum(v.astype(LD) ** 2)) / dim
    want, u = oh.sks_pairwise(x, x + v)
    assert abs(closed - want) <= 1e-17 * u
    assert abs(LD(mu.squared_kernel_sum(x, x + v)) - closed) <= 1e-12 * u
    assert mu.squared_kernel_sum(x[:1], x[:1]) == 0.0


FAR_CASES = [(m, n, 3, name) for m, n in oh.SKS_FAR_SHAPES for name in oh.SKS_FAR_OFFSETS] + [(700, 900, 33, "1e4")]


@pytest.mark.parametrize("m,n,dim,name", FAR_CASES)
def test_sks_far_from_the_origin(m, n, dim, name):
    """Against the pairwise sum of the fp64 clouds the caller passed; 1e-6 as test_sigma2_init_vs_reference."""
    from probreg_amd import math_utils as mu

    x, y = oh.far_pair(m, n, dim, oh.SKS_FAR_OFFSETS[name] if dim == 3 else 1e4)
    want = float(oh.sks_pairwise(x, y)[0])
    got = mu.squared_kernel_sum(x, y)
    print("sks far %s %dx%d dim=%d: got %.12e want %.12e rel %.2e" % (name, m, n, dim, got, want, abs(got - want) / want))
    assert abs(got - want) <= 1e-6 * want


def test_first_sigma2_of_filterreg_and_bcpd_does_not_move_with_the_clouds():
    from probreg_amd import bcpd, filterreg, synthetic

    src, tgt, _ = synthetic.rigid_pair(3000, m=2100, seed=5)
    near = filterreg.registration_filterreg(src, tgt, maxiter=0).sigma2
    far = filterreg.registration_filterreg(src + 1e5, tgt + 1e5, maxiter=0).sigma2
    print("filterreg first sigma2: %.12e, moved by 1e5 %.12e, rel %.2e" % (near, far, abs(far - near) / near))
    assert near > 1e-3 and abs(far - near) <= 1e-6 * near
    near = bcpd.CombinedBCPD(src[:500])._initialize(tgt[:400]).sigma2
    far = bcpd.CombinedBCPD(src[:500] + 1e5)._initialize(tgt[:400] + 1e5).sigma2
    print("bcpd first sigma2: %.12e, moved by 1e5 %.12e, rel %.2e" % (near, far, abs(far - near) / near))
    assert abs(far - near) <= 1e-6 * near


# --------------------------------------------------------------------------------------- rbf_kernel, inverse_multiquadric_kernel
@pytest.mark.parametrize("dim", [2, 3])
def test_rbf_and_imq_bit_equal_on_every_entry(dim):
    """16 rows x 256 columns per workgroup: 15, 16, 17, 33 rows and 255, 256, 257 columns."""
    from probreg_amd import math_utils as mu

    for m in oh.KERNEL_M:
        for n in oh.KERNEL_N:
            x, y = oh.kernel_case(m, n, dim)
            for beta in oh.RBF_BETAS:
                got, (want, fragile) = mu.rbf_kernel(x, y, beta), oh.rbf_f32(x, y, beta)
                assert not fragile.any()
                assert got.dtype == np.float32 and np.array_equal(got, want), (m, n, beta, int(np.sum(got != want)))
            for c in oh.IMQ_CS:
                got, want = mu.inverse_multiquadric_kernel(x, y, c), oh.imq_f32(x, y, c)
                assert got.dtype == np.float32 and np.array_equal(got, want), (m, n, c, int(np.sum(got != want)))


@pytest.mark.parametrize("dim", [2, 3])
def test_rbf_and_imq_square(dim):
    from probreg_amd import math_utils as mu

    x = oh.kernel_square_case(dim)
    for beta in oh.RBF_BETAS:
        k = mu.rbf_kernel(x, x, beta)
        assert np.array_equal(k, k.T) and np.all(np.diag(k) == 1.0)
        assert np.array_equal(k, oh.rbf_f32(x, x, beta)[0])
    for c in oh.IMQ_CS:
        k = mu.inverse_multiquadric_kernel(x, x, c)
        assert np.array_equal(k, k.T) and np.all(np.diag(k) == np.float32(1) / np.sqrt(np.float32(c)))
    # far enough that the exponential is below half of the smallest float32: exactly 0
    y = x[:1] + np.float32(8.0)
    assert mu.rbf_kernel(x[:1], y, 0.06)[0, 0] == 0.0 == oh.rbf_f32(x[:1], y, 0.06)[0][0, 0]


# ---------------------------------------------------------------------------------------------------------------- compute_rmse
@pytest.mark.parametrize("dim", [2, 3])
def test_rmse_small_sizes(dim):
    from probreg_amd import math_utils as mu

    worst = 0.0
    for m, n in oh.RMSE_SIZES:
        src, tgt = oh.rmse_case(m, n, dim)
        want = oh.nn_mean(src, tgt)
        got = mu.compute_rmse(src, tgt)
        worst = max(worst, abs(got - want) / want / oh.RMSE_TOL)
        assert abs(got - want) <= oh.RMSE_TOL * want, (m, n, got, want)
    print("rmse dim=%d: worst |err| / (2^-21 want) %.3f" % (dim, worst))
    src, tgt = oh.rmse_case(70, 600, dim)
    want = oh.nn_mean(src, tgt)
    assert mu.compute_rmse(tgt, tgt) == 0.0
    assert abs(mu.compute_rmse(src + 1e6, tgt + 1e6) - want) <= oh.RMSE_TOL * want


def test_rmse_many_source_blocks():
    """More than 2048 source blocks: the target is one segment.  (The cKDTree truth takes about a second.)"""
    from probreg_amd import math_utils as mu

    m, n = oh.RMSE_MANY_BLOCKS
    assert oh.nn_segments(m, n)[0] == 1
    src, tgt = oh.rmse_case(m, n, 3)
    want = oh.nn_mean(src, tgt)
    got = mu.compute_rmse(src, tgt)
    print("rmse %dx%d: |err| / (2^-21 want) %.3f" % (m, n, abs(got - want) / want / oh.RMSE_TOL))
    assert abs(got - want) <= oh.RMSE_TOL * want


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("where", [0, 207, 208, 1024])
def test_rmse_nearest_neighbour_on_a_segment_edge(dim, where):
    """1025 targets for 64 sources are five segments of 208: the one nearest neighbour of every source is the first point of the
    first segment, the last of it, the first of the second, or the last real point before the pads.  Its distances are exact
    in float32 (5 k / 8), so the mean is known: 64 fp64 square roots of exact squares and their sum, 1e-13."""
    from probreg_amd import math_utils as mu

    src, tgt, want = oh.planted_case(dim, where)
    got = mu.compute_rmse(src, tgt)
    assert abs(got - want) <= 1e-13 * want, (got, want)
