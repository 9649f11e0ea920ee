"""``probreg_amd.field.KernelField`` (csrc/field.hip) against tests/oracle_field.py, the NumPy fp64 restatement of DESIGN.md section
3.18: every output within the a-priori bound ``oracle_field.bound``, the edge cases of the kernel functions, byte repeatability
and the host-side validation."""
import numpy as np
import pytest

import oracle_field as of

pytestmark = pytest.mark.gpu

# (kernel, param, D): the four kernel functions, the two that have no dimension of their own in both
CASES = [("gaussian", 0.02, 2), ("gaussian", 0.02, 3), ("imq", 0.5, 2), ("imq", 0.5, 3), ("tps", None, 2), ("tps", None, 3)]
CASE_IDS = ["%s%dd" % (k, d) for k, _, d in CASES]
M_SIZES = (1, 2, 255, 256, 257, 1000)
Q_SIZES = (1, 63, 64, 65, 255, 257, 1000)
SLAB_M = (65535, 65536, 65537, 131073)


def _cloud(seed, n, dim, cols):
    """Control points / queries in the unit cube and weights over four decades of magnitude, both signs."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, 1.0, (n, dim))
    w = rng.normal(size=(n, cols)) * 10.0 ** rng.uniform(-2.0, 2.0, (n, 1))
    return pts, w


def _assert_within(got, want, bnd, what):
    err = np.abs(got - want)
    assert np.all(np.isfinite(got)), what
    worst = float(np.max(err / np.maximum(bnd, np.finfo(np.float64).tiny)))
    print("FIELD %-44s max err %.3g  max err / bound %.3g" % (what, float(err.max()), worst))
    assert np.all(err <= bnd), "%s: err / bound = %.3g" % (what, worst)


@pytest.mark.parametrize("cols", [1, 3, 4])
@pytest.mark.parametrize("kernel,param,dim", CASES, ids=CASE_IDS)
def test_kernel_matches_the_oracle(kernel, param, dim, cols):
    """M and Q around the wave (64), the query tile (128) and the unroll (4): the oracle and the bound are taken once per M for
    all 1000 queries, every Q is a prefix of them (a query's sum does not depend on the others)."""
    from probreg_amd.field import KernelField

    control, w = _cloud(10 * dim + cols, max(M_SIZES), dim, cols)
    queries = _cloud(77 + dim, max(Q_SIZES), dim, 1)[0]
    for m in M_SIZES:
        want = of.field(queries, control[:m], w[:m], kernel, param)
        bnd = of.bound(queries, control[:m], w[:m], kernel, param)
        field = KernelField(control[:m], w[:m], kernel, param)
        try:
            for q in Q_SIZES:
                got = field.evaluate(queries[:q])
                assert got.shape == (q, cols) and got.dtype == np.float64
                _assert_within(got, want[:q], bnd[:q], "%s D=%d C=%d M=%d Q=%d" % (kernel, dim, cols, m, q))
        finally:
            field.close()


@pytest.fixture(scope="module")
def slab_clouds():
    """One cloud per dimension for the slab-edge cases, M a prefix of it."""
    return {dim: _cloud(500 + dim, max(SLAB_M), dim, 4) + (_cloud(600 + dim, 65, dim, 1)[0],) for dim in (2, 3)}


@pytest.mark.parametrize("m", SLAB_M)
@pytest.mark.parametrize("kernel,param,dim,cols", [("gaussian", 0.02, 3, 3), ("imq", 0.5, 2, 4), ("tps", None, 2, 1),
                                                    ("tps", None, 3, 3)],
                         ids=["gaussian3d", "imq2d", "tps2d", "tps3d"])
def test_slab_edges(slab_clouds, kernel, param, dim, cols, m):
    """65 535, 65 536 (one slab, written by the kernel itself), 65 537 and 131 073 (two and three slabs, added by the second
    kernel), Q = 65: one full wave and one lane of the next tile half."""
    from probreg_amd.field import KernelField

    control, w, queries = slab_clouds[dim]
    control, w = control[:m], w[:m, :cols]
    field = KernelField(control, w, kernel, param)
    try:
        got = field.evaluate(queries)
    finally:
        field.close()
    _assert_within(got, of.field(queries, control, w, kernel, param), of.bound(queries, control, w, kernel, param),
                   "%s D=%d C=%d M=%d Q=65" % (kernel, dim, cols, m))


def _evaluate(control, w, kernel, param, queries):
    from probreg_amd.field import KernelField

    field = KernelField(control, w, kernel, param)
    try:
        return field.evaluate(queries)
    finally:
        field.close()


def test_query_on_a_control_point():
    y = np.array([[0.25, -1.5, 3.0]])
    w = np.array([[2.0, -3.0, 0.5]])
    c = 0.37
    got = _evaluate(y, w, "imq", c, y)
    _assert_within(got, w / np.sqrt(c), of.bound(y, y, w, "imq", c), "imq on a control point")
    assert np.array_equal(_evaluate(y, w, "tps", None, y), np.zeros((1, 3)))
    assert np.array_equal(_evaluate(y[:, :2], w, "tps", None, y[:, :2]), np.zeros((1, 3)))
    # ... and among other control points the point itself adds nothing
    ctrl, wts = _cloud(3, 50, 2, 2)
    got = _evaluate(ctrl, wts, "tps", None, ctrl[7:8])
    keep = np.arange(50) != 7
    _assert_within(got, of.field(ctrl[7:8], ctrl[keep], wts[keep], "tps"), of.bound(ctrl[7:8], ctrl, wts, "tps"),
                   "tps2d on one of 50 control points")


def test_spline_threshold_in_2d():
    """d2 = 0.9e-9 is below the threshold of math_utils.tps_kernel (0), 1.1e-9 above it (d2 log(d2) / 2), d2 = 1 a zero of the
    kernel; the points lie on an axis so that d2 is one exact product on both sides."""
    y = np.zeros((1, 2))
    w = np.array([[3.0]])
    x = np.array([[np.sqrt(0.9e-9), 0.0], [0.0, np.sqrt(1.1e-9)], [1.0, 0.0], [0.0, -1.0]])
    d2 = (x * x).sum(axis=1)
    assert d2[0] < 1.0e-9 < d2[1] and d2[2] == 1.0
    got = _evaluate(y, w, "tps", None, x)
    assert got[0, 0] == 0.0 and got[2, 0] == 0.0 and got[3, 0] == 0.0
    want = 3.0 * 0.5 * d2[1] * np.log(d2[1])
    assert want < 0.0 and abs(got[1, 0] - want) <= of.bound(x[1:2], y, w, "tps")[0, 0]


def test_gaussian_far_queries_are_exact_zeros():
    control, w = _cloud(5, 300, 3, 3)
    extent = float(np.max(control.max(axis=0) - control.min(axis=0)))
    far = control[:40] + 50.0 * extent * np.array([1.0, -1.0, 1.0])
    got = _evaluate(control, w, "gaussian", 0.02, far)
    assert np.all(np.isfinite(got)) and not got.any()
    assert not np.signbit(got).any()


@pytest.mark.parametrize("offset", [(0.0, 0.0, 1277.0), (1.0e6, 1.0e6, 1.0e6)], ids=["z1277", "1e6"])
@pytest.mark.parametrize("kernel,param", [("gaussian", 0.02), ("imq", 0.5), ("tps", None)])
def test_clouds_far_from_the_origin(kernel, param, offset):
    """Coordinates on the 2^-20 grid stay exact at both offsets, so the field there is the field at the origin; the bound is
    evaluated at the coordinates the kernel sees."""
    control, w = _cloud(8, 300, 3, 3)
    queries = _cloud(9, 200, 3, 1)[0]
    off = np.asarray(offset)
    control = np.round(control * 2.0 ** 20) / 2.0 ** 20 + off
    queries = np.round(queries * 2.0 ** 20) / 2.0 ** 20 + off
    assert np.array_equal((control - off) + off, control)
    got = _evaluate(control, w, kernel, param, queries)
    _assert_within(got, of.field(queries, control, w, kernel, param), of.bound(queries, control, w, kernel, param),
                   "%s at offset %s" % (kernel, offset))


@pytest.mark.parametrize("m", [1000, 65537], ids=["one_slab", "two_slabs"])
def test_results_repeat_and_do_not_depend_on_the_batch(m):
    from probreg_amd.field import KernelField

    control, w = _cloud(21, m, 3, 3)
    queries = _cloud(22, 1000, 3, 1)[0]
    field = KernelField(control, w, "gaussian", 0.02)
    try:
        first = field.evaluate(queries)
        assert field.evaluate(queries).tobytes() == first.tobytes()
        for a, b in ((37, 301), (1, 2), (129, 1000), (63, 65)):  # off the wave (64) and tile (128) edges
            assert field.evaluate(queries[a:b]).tobytes() == first[a:b].tobytes(), (a, b)
    finally:
        field.close()
    assert _evaluate(control, w, "gaussian", 0.02, queries).tobytes() == first.tobytes()  # another handle


def test_set_control_replaces_the_field():
    from probreg_amd.field import KernelField

    control, w = _cloud(31, 70, 2, 2)
    queries = _cloud(32, 90, 2, 1)[0]
    field = KernelField(control, w, "imq", 0.5)
    try:
        field.set_control(control[:33], w[:33, :1], "tps")
        got = field.evaluate(queries)
    finally:
        field.close()
    assert got.tobytes() == _evaluate(control[:33], w[:33, :1], "tps", None, queries).tobytes()


def test_validation_comes_before_any_launch():
    from probreg_amd.field import KernelField

    y, w = _cloud(41, 20, 3, 3)
    for args in ((np.zeros((20, 4)), w, "gaussian", 1.0), (y, np.ones((20, 5)), "gaussian", 1.0), (y, w, "gaussian", 0.0),
                 (y, w, "gaussian", -2.0), (y, w, "imq", 0.0)):
        with pytest.raises(ValueError):
            KernelField(*args)
    field = KernelField(y, w, "gaussian", 1.0)
    try:
        bad = y.copy()
        bad[3, 1] = np.nan
        with pytest.raises(ValueError):
            field.evaluate(bad)
        with pytest.raises(ValueError):
            field.evaluate(y[:, :2])
        empty = field.evaluate(np.zeros((0, 3)))
        assert empty.shape == (0, 3) and empty.dtype == np.float64
    finally:
        field.close()
