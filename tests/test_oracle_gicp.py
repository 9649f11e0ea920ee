"""The NumPy restatement of generalized ICP (tests/oracle_gicp.py) on the host: its per-pair inverse
against LAPACK, its system against an independently written one, and the loop cases whose decisions the GPU tests compare
exactly."""
import numpy as np
import pytest

import oracle_global_reg as og
import oracle_gicp as ogi
import oracle_icp as oi
from probreg_amd import synthetic


def _stage(m=300, r=0.05):
    """Clouds, covariances, a pose that is no identity and the matches there."""
    src, tgt, sn, tn, (rot, t) = ogi.loop_clouds(synthetic)
    src, sn = src[:m], sn[:m]
    pose = oi.pose12(og.rotation_about((1.0, 2.0, 3.0), 0.2) @ rot, t + 0.01)
    q = oi.moved(src, pose)
    idx, d2 = oi.search(q, tgt, r)
    return src, tgt, sn, tn, pose, q, idx, d2


def test_adjugate_inverse_equals_lapack():
    _, tgt, sn, tn, pose, q, idx, _ = _stage(r=np.inf)
    m = ogi.pair_matrix(pose, ogi.covariances_from_normals(sn), ogi.covariances_from_normals(tn)[idx])
    ref = pose[:9].reshape(3, 3)
    want = ogi.full(ogi.covariances_from_normals(tn)[idx]) + ref @ ogi.full(ogi.covariances_from_normals(sn)) @ ref.T
    assert np.max(np.abs(ogi.full(m) - want)) < 1.0e-15
    p = ogi.full(ogi.inverse(m))
    inv = np.linalg.inv(ogi.full(m))
    scale = np.max(np.abs(inv), axis=(1, 2))
    worst = float(np.max(np.max(np.abs(p - inv), axis=(1, 2)) / scale))
    print("adjugate against np.linalg.inv: %.3e relative; against a Cholesky inverse: %.3e" % (worst, ogi.inverse_disagreement(m)))
    assert worst < 1.0e-12 and ogi.inverse_disagreement(m) < 1.0e-12


def _independent_system(q, y, matched):
    """sum J^T J and sum J^T d with J = (-[q]x | I) built as matrices, plain NumPy sums."""
    a, g, obj = np.zeros((6, 6)), np.zeros(6), 0.0
    for m in np.nonzero(matched)[0]:
        x, yy, z = q[m]
        jac = np.zeros((3, 6))
        jac[:, :3] = -np.array([[0.0, -z, yy], [z, 0.0, -x], [-yy, x, 0.0]])
        jac[:, 3:] = np.eye(3)
        d = q[m] - y[m]
        a += jac.T @ jac
        g += jac.T @ d
        obj += d @ d
    return a, g, obj


@pytest.mark.parametrize("identity", [True, False])
def test_epsilon_one_is_half_the_unweighted_system(identity):
    """With epsilon = 1 every covariance is I, M = I + R R^T = 2 I (exactly at the identity pose) and P = I / 2."""
    src, tgt, sn, tn, pose, q, idx, d2 = _stage()
    if identity:
        pose = oi.IDENTITY.copy()
        q = oi.moved(src, pose)
        idx, d2 = oi.search(q, tgt, 0.1)
    cs, ct = ogi.covariances_from_normals(sn, 1.0), ogi.covariances_from_normals(tn, 1.0)
    assert np.array_equal(ogi.full(cs), np.tile(np.eye(3), (cs.shape[0], 1, 1)))
    s = ogi.sums(pose, q, tgt, cs, ct, idx, d2)
    matched = idx >= 0
    assert 6 < s[0] == matched.sum() < src.shape[0]
    a, g, obj = _independent_system(q, tgt[np.where(matched, idx, 0)], matched)
    got_a, got_b = oi._unpack_plane(s)
    tol = 1.0e-12 * np.max(np.abs(a))
    assert np.max(np.abs(got_a - 0.5 * a)) < tol and np.max(np.abs(-got_b - 0.5 * g)) < tol
    assert abs(s[29] - 0.5 * obj) < 1.0e-12 * obj and abs(s[1] - obj) < 1.0e-12 * obj


def test_the_sign_of_a_normal_does_not_matter():
    src, tgt, sn, tn, pose, q, idx, d2 = _stage()
    flip = np.where(np.arange(sn.shape[0]) % 2 == 0, -1.0, 1.0)[:, None]
    assert np.array_equal(ogi.covariances_from_normals(sn * flip), ogi.covariances_from_normals(sn))
    assert np.array_equal(ogi.covariances_from_normals(3.0 * tn, 0.01), ogi.covariances_from_normals(-3.0 * tn, 0.01))
    c = ogi.full(ogi.covariances_from_normals(sn))
    u = sn / np.linalg.norm(sn, axis=1)[:, None]
    assert np.max(np.abs(np.einsum("nab,nb->na", c, u) - 1.0e-3 * u)) < 1.0e-15  # eigenvalue epsilon along the normal
    assert np.max(np.abs(np.trace(c, axis1=1, axis2=2) - 2.001)) < 1.0e-15


@pytest.mark.parametrize("name,steps", zip(ogi.LOOP_CASES, (4, 5)))
def test_loop_cases(name, steps):
    """The decisions of the whole trajectory are clear of their thresholds, so a second implementation in IEEE arithmetic takes
    the same ones: matches (gaps above oracle_icp.GAP) and the last stop test (margin above 1e-9)."""
    case, res = ogi.loop_case(name, synthetic)
    deg, shift = og.pose_error(res["rot"], res["t"], *case[6])
    print("%s: n_iter %d, gap_second %.3e, gap_r %.3e, last stop-test margin %.3e, pose error %.4f deg %.2e, host solves "
          "disagree by %.3e, objective %.6e" % (name, res["n_iter"], res["gap_second"], res["gap_r"], res["margin"], deg, shift,
                                                res["disagreement"], res["objective"]))
    assert res["converged"] and res["status"] == oi.OK and res["n_iter"] == steps
    assert res["gap_second"] > oi.GAP and res["gap_r"] > oi.GAP
    assert res["margin"] > 1.0e-9
    assert deg < 0.05 and shift < 1.0e-3
    assert res["disagreement"] < 1.0e-13 and res["objective"] > 0.0


def test_six_copies_of_a_point_are_degenerate():
    _, tgt, _, tn, _, _, _, _ = _stage()
    src = np.tile(tgt[10] + 0.001, (6, 1))
    sn = np.tile(tn[10], (6, 1))
    cs, ct = ogi.covariances_from_normals(sn), ogi.covariances_from_normals(tn)
    q = oi.moved(src, oi.IDENTITY)
    idx, d2 = oi.search(q, tgt, 0.05)
    s = ogi.sums(oi.IDENTITY, q, tgt, cs, ct, idx, d2)
    assert s[0] == 6.0
    assert oi._cholesky(*oi._unpack_plane(s)) is None
    assert ogi.step(oi.IDENTITY, s) == (None, oi.DEGENERATE, 0.0)
    res = ogi.gicp(src, tgt, 0.05, cs, ct)
    assert res["n_iter"] == 0 and not res["converged"] and res["status"] == oi.DEGENERATE
    assert np.array_equal(res["pose"], oi.IDENTITY)
    few = ogi.gicp(src[:5], tgt, 0.05, cs[:5], ct)
    assert few["K"] == 5 and few["status"] == oi.DEGENERATE and few["n_iter"] == 0
