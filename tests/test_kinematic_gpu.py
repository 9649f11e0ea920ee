"""Deformable kinematic FilterReg on the GPU against its NumPy restatement
(tests/oracle_kinematic.py): skinning, the per-node-pair sums behind ``kinematic_system``, the M-step on explicit
arrays, degenerate systems, byte-repeatability, whole registrations and argument errors."""
import numpy as np
import pytest

import kinematic_cases as kc
import oracle_kinematic as ok

pytestmark = pytest.mark.gpu

IDENT = np.eye(1, 8)[0]


def _weights(pairs, vals):
    from probreg_amd import transformation as tf

    return tf.DeformableKinematicModel.make_weight(pairs, vals)


def _extent(x):
    return float(np.max(np.abs(x - x.mean(0)))) if x.shape[0] > 1 else float(np.max(np.abs(x)))


def _system_case(m, k, seed):
    """A bar with float32 E-step values near the truth, given UNSORTED, with (for k >= 3) a node index that no point
    uses, a pair segment of one point and a point whose two nodes coincide."""
    case = kc.bar(m, k, seed)
    rng = np.random.default_rng(seed + 100)
    pairs, vals = case.pairs.copy(), case.vals.copy()
    n_nodes = k
    if k >= 3 and m >= 8:
        n_nodes = k + 2
        pairs[m // 2] = (k + 1, 0)           # the only point of the ordered pair (k + 1, 0); node k is used by nobody
        pairs[m // 3] = (1, 1)               # both nodes coincide
    perm = rng.permutation(m)                # pairs in no particular order
    source, pairs, vals = case.source[perm], pairs[perm], vals[perm]
    truth = kc.true_dualquats(n_nodes)
    moved = ok.skin(truth, pairs, vals, source)
    m0 = rng.uniform(0.5, 2.0, m).astype(np.float32)
    if m >= 8:
        m0[rng.choice(m, max(m // 16, 1), replace=False)] = 0.0
    m1 = ((moved + 0.002 * rng.normal(size=(m, 3))) * m0[:, None]).astype(np.float32)
    m2 = (np.square(moved).sum(1) * m0).astype(np.float32)
    return source, pairs, vals, n_nodes, m0, m1, m2


# ---- skinning -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 5])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 1000])
def test_skinning_matches_the_restatement(m, k):
    """fp64, a few dozen operations per point: within 1e-12 of the extent."""
    from probreg_amd import transformation as tf

    case = kc.bar(m, k, seed=m + k)  # (every other point has its pair order reversed)
    model = tf.DeformableKinematicModel(case.truth, _weights(case.pairs, case.vals))
    out = model.transform(case.source)
    want = ok.skin(case.truth, case.pairs, case.vals, case.source)
    err = float(np.max(np.abs(out - want)))
    print("M = %d, K = %d: %.3g of extent %.3g" % (m, k, err, _extent(want)))
    assert out.shape == (m, 3) and err <= 1e-12 * _extent(want)


def test_host_dual_quaternion_helpers_match_the_restatement():
    from probreg_amd import transformation as tf

    rng = np.random.default_rng(5)
    for _ in range(5):
        tw = rng.normal(size=6) * 0.3
        np.testing.assert_allclose(tf.dualquat_from_twist(tw), ok.dq_from_twist(tw), atol=1e-15)
        a, b = ok.dq_from_twist(rng.normal(size=6)), ok.dq_from_twist(rng.normal(size=6))
        np.testing.assert_allclose(tf.dualquat_mul(a, b), ok.dq_mul(a, b), atol=1e-15)
    np.testing.assert_array_equal(tf.dualquat_from_twist(np.r_[1e-9, 0, 0, 1, 2, 3])[:4], [1, 0, 0, 0])
    assert tf.dualquat_identity(3).shape == (3, 8)
    th = np.deg2rad(30.0)
    rot = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    np.testing.assert_allclose(tf.dualquat_from_rt(rot, [0, 0, 0.3]), kc.reference_example().truth[1], atol=1e-15)


def test_dualquat_from_rt_on_half_turns_round_trips_through_skinning():
    """Rotations of about 180 degrees about each axis take the three diagonal-pivot branches of dualquat_from_rt
    (the trace is near -1); the skinned points are R x + t."""
    from probreg_amd import transformation as tf

    rng = np.random.default_rng(8)
    pts = rng.normal(size=(65, 3))
    weights = _weights(np.zeros((65, 2), dtype=np.int32), np.tile(np.float32([0.25, 0.75]), (65, 1)))
    for axis in range(3):
        for ang in (np.pi, np.pi - 1e-3, np.pi + 0.2):
            a = rng.normal(size=3) * 0.05
            a[axis] = 1.0
            a /= np.linalg.norm(a)
            kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            rot = np.identity(3) + np.sin(ang) * kx + (1.0 - np.cos(ang)) * kx @ kx
            assert int(np.argmax([np.trace(rot), rot[0, 0], rot[1, 1], rot[2, 2]])) == axis + 1
            t = rng.normal(size=3)
            q = tf.dualquat_from_rt(rot, t)
            assert abs(np.linalg.norm(q[:4]) - 1.0) < 1e-14
            out = tf.DeformableKinematicModel([q], weights).transform(pts)
            assert np.max(np.abs(out - (pts @ rot.T + t))) < 1e-12 * _extent(pts)


# ---- the sums behind kinematic_system -----------------------------------------------------------------------------------
@pytest.mark.parametrize("reference_form", [False, True])
@pytest.mark.parametrize("m,k", [(1, 2), (64, 2), (65, 3), (257, 3), (3000, 8)])
def test_kinematic_system_matches_the_restatement(m, k, reference_form):
    """Every entry within 1e-10 max|A| and 1e-10 max|b|: an fp64 sum of at most 3000 terms is bounded by about
    3000 eps relative, which leaves 100x and more."""
    from probreg_amd import filterreg as fr

    source, pairs, vals, n_nodes, m0, m1, m2 = _system_case(m, k, seed=7 * m + k)
    for w in (0.0, 0.1):
        a, b = fr.kinematic_system(source, m + 3, (m0, m1, m2), _weights(pairs, vals), 2e-3, w, reference_form)
        # (kinematic_system sizes the system by the largest index in use)
        kk = int(pairs.max()) + 1
        wa, wb = ok.kinematic_system(source, m + 3, m0, m1, pairs, vals, kk, 2e-3, w, reference_form)
        ea, eb = float(np.max(np.abs(a - wa))), float(np.max(np.abs(b - wb)))
        print("(M, K) = (%d, %d) w = %g ref = %s: A %.3g of %.3g, b %.3g of %.3g"
              % (m, k, w, reference_form, ea, np.max(np.abs(wa)), eb, np.max(np.abs(wb))))
        assert a.shape == (6 * kk, 6 * kk) and np.isfinite(a).all() and np.isfinite(b).all()
        assert ea <= 1e-10 * np.max(np.abs(wa))
        assert eb <= 1e-10 * np.max(np.abs(wb))


# ---- the M-step on explicit arrays --------------------------------------------------------------------------------------
def _mstep(case_args, reference_form=False, w=0.1, with_m2=True, n_nodes=None):
    from probreg_amd import filterreg as fr
    from probreg_amd import transformation as tf

    source, pairs, vals, kk, m0, m1, m2 = case_args
    kk = kk if n_nodes is None else n_nodes
    start = kc.true_dualquats(kk, motion=0.5)
    model = tf.DeformableKinematicModel(start, _weights(pairs, vals))
    es = fr.EstepResult(m0, m1, m2 if with_m2 else None, None)
    target = np.zeros((source.shape[0] + 3, 3))
    res = fr.DeformableKinematicFilterReg._maximization_step(source, target, es, model, 2e-3, w,
                                                             reference_form=reference_form)
    want = ok.maximization_step(source, target.shape[0], m0, m1, m2 if with_m2 else None, start, pairs, vals, 2e-3, w,
                                reference_form=reference_form)
    return res, want


def _well_conditioned_case(m, k, seed):
    """The bar of the sums test without its degenerate additions: every node in use, every segment well filled."""
    case = kc.bar(m, k, seed)
    rng = np.random.default_rng(seed + 100)
    perm = rng.permutation(m)
    source, pairs, vals = case.source[perm], case.pairs[perm], case.vals[perm]
    moved = case.moved[perm]
    m0 = rng.uniform(0.5, 2.0, m).astype(np.float32)
    m0[rng.choice(m, m // 16, replace=False)] = 0.0
    m1 = ((moved + 0.002 * rng.normal(size=(m, 3))) * m0[:, None]).astype(np.float32)
    m2 = (np.square(moved).sum(1) * m0).astype(np.float32)
    return source, pairs, vals, k, m0, m1, m2


@pytest.mark.parametrize("m,k", [(257, 3), (3000, 8)])
def test_maximization_step_matches_the_restatement(m, k):
    """Equal inner iteration count; dual quaternions, q and sigma2 within 1e-8 relative (cond(A) <= 2e4 times the
    1e-10 of the sums, with margin)."""
    res, want = _mstep(_well_conditioned_case(m, k, seed=31 + m))
    dq = res.transformation.dualquats
    e_dq = float(np.max(np.abs(dq - want.dualquats))) / float(np.max(np.abs(want.dualquats)))
    e_q = abs(res.q - want.q) / abs(want.q)
    e_s = abs(res.sigma2 - want.sigma2) / want.sigma2
    print("(M, K) = (%d, %d): %d / %d inner iterations, dualquats %.3g, q %.3g, sigma2 %.3g"
          % (m, k, res.transformation.inner_iterations, want.n_iter, e_dq, e_q, e_s))
    assert res.transformation.inner_iterations == want.n_iter
    assert e_dq <= 1e-8 and e_q <= 1e-8 and e_s <= 1e-8


@pytest.mark.parametrize("name", ["single_point", "unused_node", "one_point_segment"])
def test_degenerate_systems_agree_on_points_and_q(name):
    """The twists of a rank-deficient system are not unique (minimum norm picks one): the skinned points and q are
    compared, to the 1e-8 of the well-conditioned M-step (points against the extent, q against its value at zero
    increments); the dual quaternion of a node nobody uses comes back bit-identical; nothing is NaN."""
    if name == "single_point":
        args, kk = _system_case(1, 2, seed=3), 2
    elif name == "unused_node":
        s, p, v, _, m0, m1, m2 = _well_conditioned_case(257, 3, seed=9)
        args, kk = (s, p, v, 4, m0, m1, m2), 4  # node 3 has no points
    else:
        s, p, v, _, m0, m1, m2 = _well_conditioned_case(257, 3, seed=10)
        p = p.copy()
        p[100] = (2, 0)  # the only point of the ordered pair (2, 0)
        args, kk = (s, p, v, 3, m0, m1, m2), 3
    res, want = _mstep(args, n_nodes=kk)
    source, pairs, vals = args[0], args[1], args[2]
    dq = res.transformation.dualquats
    assert np.isfinite(dq).all() and np.isfinite(res.q) and np.isfinite(res.sigma2)
    got_pts = res.transformation.transform(source)
    want_pts = ok.skin(want.dualquats, pairs, vals, source)
    scale = max(_extent(want_pts), 1e-300)
    e_p = float(np.max(np.abs(got_pts - want_pts))) / scale
    # (a single point is fitted exactly, q -> 0: the scale of q is its value at zero increments)
    q0 = ok.initial_q(source, source.shape[0] + 3, args[4], args[5], pairs, vals, kk, 2e-3, 0.1)
    e_q = abs(res.q - want.q) / q0
    print("%s: points %.3g of the extent, q %.3g of its initial value, %d / %d inner iterations"
          % (name, e_p, e_q, res.transformation.inner_iterations, want.n_iter))
    assert e_p <= 1e-8 and e_q <= 1e-8
    if name == "unused_node":
        assert dq[3].tobytes() == kc.true_dualquats(4, motion=0.5)[3].tobytes()


# ---- byte-repeatability ---------------------------------------------------------------------------------------------------
def test_mstep_and_registration_repeat_byte_for_byte():
    from probreg_amd import filterreg as fr

    args = _well_conditioned_case(3000, 8, seed=77)
    a, _ = _mstep(args)
    b, _ = _mstep(args)
    assert a.transformation.dualquats.tobytes() == b.transformation.dualquats.tobytes()
    assert a.q == b.q and a.sigma2 == b.sigma2

    case = kc.bar(600, 3, 5)
    runs = []
    for _ in range(2):
        reg = fr.DeformableKinematicFilterReg(case.source, _weights(case.pairs, case.vals), 1e-3, update_sigma2=True)
        res = reg.registration(case.target, w=0.1, maxiter=5, tol=-1)
        runs.append((res.transformation.dualquats.tobytes(), res.sigma2, res.q,
                     res.transformation.transform(case.source).tobytes()))
    assert runs[0] == runs[1]


# ---- whole registrations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0.0, 0.1])
@pytest.mark.parametrize("mode", ["fixed", "update"])
@pytest.mark.parametrize("m,k,n,seed", [(1500, 4, 1500, 3), (1500, 4, 1200, 4), (600, 3, 600, 5)])
def test_registration_recovers_the_motion(m, k, n, seed, mode, w):
    """12 iterations, tol = -1: the RMS distance to the truth ends at most 0.25 x its initial value (the restatement on
    the oracle's lattice E-step measures 0.03 to 0.11 with sigma2 = 1e-3 fixed, 0.009 to 0.015 updating from 3e-3)."""
    from probreg_amd import filterreg as fr

    case = kc.bar(m, k, seed, n=n)
    sigma2, update = (1e-3, False) if mode == "fixed" else (3e-3, True)
    reg = fr.DeformableKinematicFilterReg(case.source, _weights(case.pairs, case.vals), sigma2, update_sigma2=update)
    res = reg.registration(case.target, w=w, maxiter=12, tol=-1)
    start = kc.rms(case.source, case.moved)
    end = kc.rms(res.transformation.transform(case.source), case.moved)
    print("(%d, %d, %d, %d) %s w = %g: rms %.4g -> %.4g (%.3f), sigma2 %.3g" % (m, k, n, seed, mode, w, start, end, end / start, res.sigma2))
    assert end <= 0.25 * start


def _cpu_loop(case, iters, sigma2, w):
    hist = []
    ok.registration(case.source, case.target, case.pairs, case.vals, case.n_nodes, sigma2, False, w, maxiter=iters, tol=-1,
                    history=hist)
    return hist


def test_registration_matches_the_cpu_loop():
    """(600, 3, 600, 5), 5 iterations, fixed sigma2, against oracle.filterreg_numpy.expectation_step + the restatement:
    FilterReg's north-star tolerance, skinned points within 1e-4 of the extent."""
    from probreg_amd import filterreg as fr

    case = kc.bar(600, 3, 5)
    hist = _cpu_loop(case, 5, 1e-3, 0.0)
    reg = fr.DeformableKinematicFilterReg(case.source, _weights(case.pairs, case.vals), 1e-3)
    res = reg.registration(case.target, w=0.0, maxiter=5, tol=-1)
    want = ok.skin(hist[-1][0], case.pairs, case.vals, case.source)
    got = res.transformation.transform(case.source)
    err = float(np.max(np.abs(got - want))) / _extent(want)
    print("device loop vs CPU loop after 5 iterations: %.3g of the extent; q %.6g vs %.6g" % (err, res.q, hist[-1][2]))
    assert err <= 1e-4


def test_device_loop_matches_the_public_step_by_step_path():
    """transform -> expectation_step -> maximization_step over 3 iterations, same tolerance as against the CPU loop."""
    from probreg_amd import filterreg as fr

    case = kc.bar(600, 3, 5)
    weights = _weights(case.pairs, case.vals)
    reg = fr.DeformableKinematicFilterReg(case.source, weights, 1e-3)
    res = reg.registration(case.target, w=0.1, maxiter=3, tol=-1)
    step = fr.DeformableKinematicFilterReg(case.source, weights, 1e-3)
    for _ in range(3):
        ts = step._tf_result.transform(case.source)
        es = step.expectation_step(ts, case.target, case.target, 1e-3, False)
        out = step.maximization_step(ts, case.target, es, w=0.1)
        step._tf_result = out.transformation
    want = step._tf_result.transform(case.source)
    got = res.transformation.transform(case.source)
    err = float(np.max(np.abs(got - want))) / _extent(want)
    print("device loop vs step by step after 3 iterations: %.3g of the extent" % err)
    assert err <= 1e-4


def test_device_loop_matches_step_by_step_on_a_morton_sorted_source():
    """From 4096 source points on, the plan stores the source in Morton order and every per-point array of the
    kinematic sums goes through that permutation: (5000, 4), 3 iterations against the public step-by-step path (which
    works on explicit arrays in the caller's order), same tolerance, and the motion is recovered."""
    from probreg_amd import filterreg as fr

    case = kc.bar(5000, 4, 6)
    weights = _weights(case.pairs, case.vals)
    res = fr.DeformableKinematicFilterReg(case.source, weights, 1e-3).registration(case.target, w=0.1, maxiter=3, tol=-1)
    step = fr.DeformableKinematicFilterReg(case.source, weights, 1e-3)
    for _ in range(3):
        ts = step._tf_result.transform(case.source)
        es = step.expectation_step(ts, case.target, case.target, 1e-3, False)
        step._tf_result = step.maximization_step(ts, case.target, es, w=0.1).transformation
    want = step._tf_result.transform(case.source)
    got = res.transformation.transform(case.source)
    err = float(np.max(np.abs(got - want))) / _extent(want)
    start, end = kc.rms(case.source, case.moved), kc.rms(got, case.moved)
    print("Morton-sorted device loop vs step by step: %.3g of the extent; rms %.4g -> %.4g" % (err, start, end))
    assert err <= 1e-4
    assert end < 0.5 * start


def test_feature_fn_driver_and_callbacks():
    """A non-identity feature_fn takes the base driver (transform and _maximization_step only); callbacks see every
    iteration's model and `tol` stops on |q - q_prev|."""
    from probreg_amd import filterreg as fr

    case = kc.bar(600, 3, 5)
    weights = _weights(case.pairs, case.vals)
    seen = []
    reg = fr.DeformableKinematicFilterReg(None, weights, 1e-3)
    reg.set_source(case.source)
    reg.set_callbacks([lambda t: seen.append(t.dualquats.copy())])
    res = reg.registration(case.target, maxiter=3, tol=-1, feature_fn=lambda x: 1.0 * x)
    assert len(seen) == 3 and seen[-1].tobytes() == res.transformation.dualquats.tobytes()
    dev = fr.DeformableKinematicFilterReg(case.source, weights, 1e-3).registration(case.target, maxiter=3, tol=-1)
    err = float(np.max(np.abs(dev.transformation.transform(case.source) - res.transformation.transform(case.source))))
    assert err <= 1e-4 * _extent(case.moved)
    early = fr.DeformableKinematicFilterReg(case.source, weights, 1e-3).registration(case.target, maxiter=12, tol=1e30)
    assert early.transformation.dualquats.tobytes() == fr.DeformableKinematicFilterReg(
        case.source, weights, 1e-3).registration(case.target, maxiter=2, tol=-1).transformation.dualquats.tobytes()


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from probreg_amd import filterreg as fr
    from probreg_amd import transformation as tf

    case = kc.bar(64, 3, 1)
    weights = _weights(case.pairs, case.vals)
    with pytest.raises(ValueError):
        fr.DeformableKinematicFilterReg(case.source[:, :2], weights, 1e-3)                    # dim != 3
    with pytest.raises(ValueError):
        fr.DeformableKinematicFilterReg(case.source[:50], weights, 1e-3)                      # wrong length
    bad = case.pairs.copy()
    bad[5, 0] = -1
    with pytest.raises(ValueError):
        fr.DeformableKinematicFilterReg(case.source, _weights(bad, case.vals), 1e-3)          # index outside [0, K)
    with pytest.raises(ValueError):
        tf.DeformableKinematicModel(tf.dualquat_identity(2), weights)                         # 3 nodes named, 2 given
    with pytest.raises(ValueError):
        tf.DeformableKinematicModel(tf.dualquat_identity(3), weights).transform(case.source[:10])
    with pytest.raises(ValueError):
        fr.kinematic_system(case.source[:, :2], 64, (np.ones(64), case.source), weights, 1e-3)

    plan = fr._Plan()
    try:
        plan.set_source(case.source)
        plan.set_target(case.target)
        plan.set_skinning(case.pairs, case.vals, 3)
        plan.set_dualquats(case.truth)
        high = case.pairs.copy()
        high[7, 1] = 3
        with pytest.raises(ValueError):
            plan.set_skinning(high, case.vals, 3)
        with pytest.raises(ValueError):
            plan.set_skinning(case.pairs[:10], case.vals[:10], 3)
        # the plan is still usable, with the skinning it had
        np.testing.assert_array_equal(plan.get_dualquats(), case.truth)
        plan.kinematic_estep(1e-3)
        m0, _, _ = plan.get_estep(False)
        assert m0.shape == (64,) and np.isfinite(m0).all() and m0.max() > 0
        nsum = plan.kinematic_normal_sums(1e-3, 0.0, False)
        assert np.isfinite(nsum).all()
    finally:
        plan.close()
