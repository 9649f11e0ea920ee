"""The restatement of fast global registration (tests/oracle_fgr.py) pinned on facts it cannot get
wrong by construction, and the quality condition of the method stated on the restatement alone.  No GPU."""
import numpy as np
import pytest

import fgr_cases as fc
import oracle_fgr as of
import oracle_global_reg as og
import oracle_icp as oi


def test_exact_correspondences_give_the_true_pose():
    src, tgt, corr, rot, t = fc.exact_case()
    for kw in (dict(), dict(tuple_test=False), dict(use_absolute_scale=True, maximum_correspondence_distance=0.05)):
        r = of.fgr(src, tgt, corr, **kw)
        assert r["status"] == of.OK and r["n_iter"] == 64
        err = max(float(np.max(np.abs(r["rot"] - rot))), float(np.max(np.abs(r["t"] - t))))
        print("exact %s: err = %.3e, objective %.3e" % (kw, err, r["objective"]))
        assert err <= 1.0e-12
        assert np.all(r["weights"] > 1.0 - 1.0e-12)


def test_twist_convention_is_the_icp_restatements():
    rng = np.random.default_rng(5)
    for _ in range(20):
        x = rng.uniform(-0.7, 0.7, 6)
        pose = oi.pose12(og.rotation_about(rng.normal(size=3), rng.uniform(0.0, 3.0)), rng.normal(size=3))
        rot, t = oi._delta_from_x(x)
        want = oi._update(pose, rot, t)
        got = of.compose(of.delta_from_x(x), pose)
        assert np.max(np.abs(got - want)) <= 4.0 * 2.0 ** -52 * max(1.0, np.max(np.abs(want)))
    # the sign of the Jacobian: a small twist x moves s by omega x s + v
    s = rng.uniform(-1.0, 1.0, (4, 3))
    x = rng.uniform(-1.0, 1.0, 6) * 1.0e-7
    moved = of.moved(s, of.delta_from_x(x))
    lin = np.einsum("kab,b->ka", of.jacobian(s), x)
    assert np.max(np.abs((moved - s) - lin)) < 1.0e-13
    # and the same system as the point-to-plane / generalized ICP solve
    a = rng.normal(size=(6, 6))
    a = a @ a.T + np.eye(6)
    b = rng.normal(size=6)
    assert np.max(np.abs(of.cholesky(a, b) - oi._cholesky(a, b))) < 1.0e-12
    assert of.cholesky(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, 1.0e-13]), b) is None and of.PIVOT == oi.PIVOT


def test_draws_are_section_3_13s():
    assert of.draw is og.draw
    src, tgt, corr, _, _ = fc.case(600, 0.5, 0)
    r = fc.reference(600, 0.5, 0)
    p, q = of.pairs(src, tgt, corr, r["mean_p"], r["mean_q"], r["scale_global"])
    tri = og.draw(0, np.arange(r["n_trials"], dtype=np.uint64), 600)
    ok = of.trial_passes(p, q, tri, 0.95)
    assert ok[-1] and int(ok.sum()) == 1000 == r["n_tuples"]
    assert np.array_equal(tri[ok].reshape(-1), r["used"])
    repeated = (tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2])
    assert repeated.any() and not ok[repeated].any()      # strict inequalities: a repeated correspondence fails by itself
    assert of.tuples(p, q, 0, block=977)[1:] == (r["n_tuples"], r["n_trials"])
    assert np.array_equal(of.tuples(p, q, 0, block=977)[0], r["used"])


def test_weight_and_schedule():
    assert of.weight(0.37, 0.0) == 1.0 and of.weight(0.37, 0.37) == 0.25
    mu, seq = 1.0, []
    for i in range(64):
        mu = of.next_mu(mu, i)
        seq.append(mu)
    want, m = [], 1.0
    for i in range(64):
        if i % 4 == 0 and m > 0.025:
            m = m / 1.4
        want.append(m)
    assert seq == want
    # eleven divisions: 1.4^-11 = 0.0247 is the first value not above 0.025; they happen after iterations 0, 4, .., 40
    assert len(set(seq)) == 11 and seq[0] == 1.0 / 1.4 and seq[39] > 0.025 >= seq[40] == seq[63]
    assert abs(seq[63] - 1.4 ** -11) < 1.0e-15
    r = fc.reference(600, 0.5, 0)
    assert r["mus"].tolist() == seq and r["mu"] == seq[-1]
    assert of.next_mu(1.0, 0, decrease_mu=False) == 1.0


def test_objective_is_reported_and_decides_nothing():
    p, q, pose, mu = fc.pair_cloud(65)
    s = of.sums(p, q, pose, mu)
    terms, l = of.pair_terms(p, q, pose, mu)
    r = of.moved(p, pose) - q
    r2 = np.sum(r * r, axis=1)
    assert abs(s[27] - np.sum(l * r2 + mu * (1.0 - np.sqrt(l)) ** 2)) < 1.0e-12
    a, b = of._unpack(s)
    jac = of.jacobian(of.moved(p, pose))
    assert np.max(np.abs(a - np.einsum("k,kai,kaj->ij", l, jac, jac))) < 1.0e-12
    assert np.max(np.abs(-b - np.einsum("k,kai,ka->i", l, jac, r))) < 1.0e-12


@pytest.mark.parametrize("c,wrong,seed", fc.QUALITY)
def test_quality_on_mostly_wrong_correspondences(c, wrong, seed):
    """The pose is within 0.5 degrees and 5e-3 of the truth with 50, 70 and 80 % of the correspondences wrong.  Measured here:
    at most 0.108 degrees and 5.0e-4 over the nine cases."""
    _, _, _, rot, t = fc.case(c, wrong, seed)
    r = fc.reference(c, wrong, seed)
    deg, shift = og.pose_error(r["rot"], r["t"], rot, t)
    print("C = %d, %.0f %% wrong, seed %d: %d tuples in %d trials, %.4f deg, %.2e" % (c, 100 * wrong, seed, r["n_tuples"],
                                                                                     r["n_trials"], deg, shift))
    assert r["status"] == of.OK and r["n_iter"] == 64
    assert deg <= fc.QUALITY_DEG and shift <= fc.QUALITY_SHIFT


def test_without_the_tuple_test_at_70_percent_wrong():
    src, tgt, corr, rot, t = fc.case(800, 0.7, 1)
    r = fc.reference(800, 0.7, 1, tuple_test=False)
    deg, shift = og.pose_error(r["rot"], r["t"], rot, t)
    print("no tuple test: %.4f deg, %.2e" % (deg, shift))
    assert np.array_equal(r["used"], np.arange(800)) and deg <= fc.QUALITY_DEG and shift <= fc.QUALITY_SHIFT


def test_the_trial_limit_ends_the_search_of_one_case():
    r = fc.reference(1000, 0.8, 0)
    assert r["n_trials"] == 100 * 1000 and 0 < r["n_tuples"] < 1000 and r["used"].shape[0] == 3 * r["n_tuples"]
