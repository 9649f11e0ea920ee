"""tests/oracle_field.py, the restatement of the kernel field, pinned on what the unmodified reference
computes (tests/golden/field_golden.npz, written by tests/golden/make_field_golden.py).  Host only."""
import os

import numpy as np
import pytest

import oracle_field as of
from conftest import GOLDEN_DIR, Golden


@pytest.fixture(scope="module")
def golden():
    return Golden(os.path.join(GOLDEN_DIR, "field_golden.npz"))


def test_nonrigid_cpd_field_moves_the_control_points_like_the_reference(golden):
    """control + f(control) is the reference's ``transform(control)`` up to its float32 kernel matrix: measured 4.7e-5 at
    worst against a bound of 9e-4 (max |w| = 107 for displacements of 0.1)."""
    c = golden.case("cpd")
    moved = c["control"] + of.field(c["control"], c["control"], c["w"], "gaussian", c["beta"])
    err = np.abs(moved - c["moved"])
    bnd = of.f32_kernel_bound(c["control"], c["control"], c["w"], "gaussian", c["beta"])
    print("cpd: max err %.3g, max bound %.3g, max err / bound %.3g" % (err.max(), bnd.max(), (err / bnd).max()))
    assert np.all(err <= bnd)
    assert np.abs(c["w"]).max() > 50.0  # (the cancellation that makes fp64 necessary is in the fixture)


@pytest.mark.parametrize("dim", [2, 3])
def test_tps_field_moves_other_points_like_the_reference(golden, dim):
    c = golden.case("tps%d" % dim)
    ctrl, pts = c["control"], c["points"]
    u = np.linalg.svd(np.c_[np.ones((ctrl.shape[0], 1)), ctrl])[0]
    nv = u[:, dim + 1:] @ c["v"]
    moved = c["a"][0] + pts @ c["a"][1:] + of.field(pts, ctrl, nv, "tps")
    err = np.abs(moved - c["moved"])
    bnd = of.f32_kernel_bound(pts, ctrl, nv, "tps")
    print("tps%d: max err %.3g, max bound %.3g, max err / bound %.3g" % (dim, err.max(), bnd.max(), (err / bnd).max()))
    assert np.all(err <= bnd)


# max |G32 W_b - v_hat| / max |v_hat| of the reference's own M-step, measured on the fixture; the
# tests assert four times these, the margin is for LAPACK builds.  The reference inverts G in float32: on the voxel means
# (cond(G) = 7.8e11) its v_hat is not the solution of its own system any more (it differs from a stable solve by 0.4 max |v_hat|),
# so that figure pins the fixture and not the identity; on the well-separated grid (cond(G) = 34) the identity holds to float32.
BCPD_MEASURED = {"bcpd": 38.95, "bcpd_grid": 6.76e-8}


@pytest.mark.parametrize("case", sorted(BCPD_MEASURED))
def test_bcpd_weights_reproduce_v_hat_through_the_float32_kernel(golden, case):
    c = golden.case(case)
    w_b = of.bcpd_weights(c["s2s2"], c["lmd"], c["nu"], c["residual"], c["v_hat"])
    g32 = of.kernel_matrix_f32(c["control"], c["control"], "imq", 1.0).astype(np.float64)
    res = np.abs(g32 @ w_b - c["v_hat"]).max() / np.abs(c["v_hat"]).max()
    print("%s: max |G32 W_b - v_hat| / max |v_hat| = %.4g" % (case, res))
    assert res <= 4.0 * BCPD_MEASURED[case]


@pytest.mark.parametrize("case", sorted(BCPD_MEASURED))
def test_bcpd_identity_with_a_stable_solve(golden, case):
    """With v_hat from a stable solve of the same system, (lmd I + s2s2 G diag(nu)) v = s2s2 G (nu o residual), the identity
    v = G W_b holds to rounding: the algebra is right, whatever the reference's float32 inverse does to it.  The bound is the
    backward error of the solve, cond(A) 2^-53 with a factor 64 for LAPACK's constants."""
    c = golden.case(case)
    g = of.kernel_value(of.sqdist(c["control"], c["control"]), "imq", 1.0, 3)
    a = c["lmd"] * np.identity(g.shape[0]) + c["s2s2"] * g * c["nu"][None, :]
    v = np.linalg.solve(a, c["s2s2"] * g @ (c["nu"][:, None] * c["residual"]))
    w_b = of.bcpd_weights(c["s2s2"], c["lmd"], c["nu"], c["residual"], v)
    res = np.abs(of.field(c["control"], c["control"], w_b, "imq", 1.0) - v).max() / np.abs(v).max()
    print("%s: stable solve, max |G W_b - v| / max |v| = %.3g, cond(A) = %.3g" % (case, res, np.linalg.cond(a)))
    assert res <= 64.0 * np.linalg.cond(a) * 2.0 ** -53


def test_field_sums_in_slab_order():
    """Two slabs: the result is (slab 0 summed from 0) + (slab 1 summed from 0), not one running sum."""
    rng = np.random.default_rng(0)
    m = of.SLAB + 3
    y, w, x = rng.normal(size=(m, 2)), rng.normal(size=(m, 1)), rng.normal(size=(2, 2))
    k = of.kernel_value(of.sqdist(x, y), "imq", 0.5, 2) * w[None, :, 0]
    want = np.cumsum(k[:, :of.SLAB], axis=1)[:, -1] + np.cumsum(k[:, of.SLAB:], axis=1)[:, -1]
    assert np.array_equal(of.field(x, y, w, "imq", 0.5)[:, 0], want)


def test_kernel_definitions():
    d2 = np.array([0.0, 0.9e-9, 1.1e-9, 1.0, 4.0])
    assert np.array_equal(of.kernel_value(d2, "tps", None, 2)[[0, 1, 3]], [0.0, 0.0, 0.0])
    assert of.kernel_value(d2, "tps", None, 2)[2] == 0.5 * 1.1e-9 * np.log(1.1e-9)
    assert np.array_equal(of.kernel_value(d2, "tps", None, 3), -np.sqrt(d2))
    assert np.array_equal(of.kernel_value(d2, "gaussian", 2.0, 3), np.exp(-d2 / 4.0))  # 2 beta, not 2 beta^2
    assert np.array_equal(of.kernel_value(d2, "imq", 1.0, 3), 1.0 / np.sqrt(d2 + 1.0))


def test_base_class_warp_is_transform():
    """Rigid and affine results are functions of the point alone: ``warp`` is ``transform``, byte for byte."""
    from probreg_amd import transformation as tf

    rng = np.random.default_rng(1)
    pts = rng.normal(size=(50, 3))
    rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    for t in (tf.RigidTransformation(rot, rng.normal(size=3), 1.3), tf.AffineTransformation(rng.normal(size=(3, 3)), rng.normal(size=3))):
        assert t.warp(pts).tobytes() == t.transform(pts).tobytes()


def test_combined_warp_without_a_field():
    from probreg_amd import transformation as tf

    pts = np.random.default_rng(2).normal(size=(10, 3))
    t = tf.CombinedTransformation(np.identity(3), np.array([0.1, 0.2, 0.3]), 1.1)  # v = 0: a similarity, any points will do
    assert t.warp(pts[:4]).tobytes() == t.transform(pts[:4]).tobytes()
    t = tf.CombinedTransformation(np.identity(3), np.zeros(3), 1.0, 0.01 * pts)
    with pytest.raises(ValueError, match="field"):
        t.warp(pts[:4])


def test_kernel_field_checks_its_arguments_before_it_needs_a_gpu():
    from probreg_amd.field import KernelField

    y, w = np.zeros((5, 3)), np.ones((5, 3))
    for args in ((np.zeros((5, 4)), w, "gaussian", 1.0), (y, np.ones((5, 5)), "gaussian", 1.0), (y, np.ones((4, 3)), "imq", 1.0),
                 (y, w, "gaussian", 0.0), (y, w, "gaussian", -1.0), (y, w, "gaussian", None), (y, w, "imq", 0.0),
                 (y, w, "imq", float("nan")), (y, w, "tps", 1.0), (y, w, "cubic", 1.0),
                 (np.full((5, 3), np.nan), w, "tps", None), (y, np.full((5, 3), np.inf), "tps", None)):
        with pytest.raises(ValueError):
            KernelField(*args)
