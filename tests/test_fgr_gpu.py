"""Fast global registration on the GPU (probreg_amd.global_reg.registration_fgr / FgrPlan, csrc/fgr.hip) against its
restatement (tests/oracle_fgr.py), stage by stage and end to end.

Means, scale, the accepted tuples, the trial count, the 28 sums, the sequence of mu and the step count are compared to the
last bit.  A step's pose gets the bound of the ICP step tests (8 x the disagreement of two host solves of the same sums,
floor 1e-12).  The pose and the weights after the 64-step loop get 16 x what the restatement itself moves by when every pose
entry is perturbed by one ulp after each step (see test_loop_equals_the_restatement).
"""
import numpy as np
import pytest

import fgr_cases as fc
import oracle_fgr as of
import oracle_global_reg as og

pytestmark = pytest.mark.gpu


def _gr():
    from probreg_amd import global_reg
    return global_reg


def _plan(src, tgt, corr, use_absolute_scale=False):
    plan = _gr().FgrPlan()
    plan.set_clouds(src, tgt)
    plan.set_correspondences(corr)
    return plan, plan.normalise(use_absolute_scale)


def _ref_pairs(src, tgt, corr, use_absolute_scale=False):
    mean_p, mean_q, _, sg, _ = of.normalise(src, tgt, use_absolute_scale)
    return of.pairs(src, tgt, corr, mean_p, mean_q, sg)


# ----------------------------------------------------------------------------------------------------------- normalise
@pytest.mark.parametrize("m,n,shift", [(1, 1, 0.0), (63, 64, 0.0), (64, 65, 0.0), (65, 4097, 0.0), (4097, 63, 2.0 ** 20),
                                       (1, 65, 2.0 ** 20)])
def test_means_and_scale_equal_the_restatement_to_the_last_bit(m, n, shift):
    src, tgt = fc.normalise_cloud(m, shift), fc.normalise_cloud(n, 0.0, seed=1)
    corr = np.stack([np.arange(5) % m, np.arange(5) % n], axis=1).astype(np.int32)
    plan, (mean_p, mean_q, scale) = _plan(src, tgt, corr)
    try:
        ref = of.normalise(src, tgt)
        assert mean_p.tobytes() == ref[0].tobytes() and mean_q.tobytes() == ref[1].tobytes()
        assert np.float64(scale).tobytes() == np.float64(ref[2]).tobytes()
        if m == 1 and n == 1:   # two single points: scale 0, no pairs; the later stages say so instead of dividing by it
            assert scale == 0.0
            with pytest.raises(_gr()._lib.ProbregHipError):
                plan.tuples()
    finally:
        plan.close()


def test_a_correspondence_outside_the_clouds_is_an_error_of_the_handle():
    src, tgt, corr, _, _ = fc.exact_case()
    bad = corr.copy()
    bad[7, 1] = tgt.shape[0]
    plan = _gr().FgrPlan()
    try:
        plan.set_clouds(src, tgt)
        plan.set_correspondences(bad)
        with pytest.raises(ValueError):
            plan.normalise()
        plan.set_correspondences(corr)
        plan.normalise()
        with pytest.raises(ValueError):
            plan.set_used(np.array([0, 1, corr.shape[0]], dtype=np.int32))
    finally:
        plan.close()


# -------------------------------------------------------------------------------------------------------------- tuples
def _tuples_case(name):
    src, tgt, corr, _, _ = fc.case(600, 0.5, 0)
    if name == "c60_cap7":
        return src, tgt, corr[:60], dict(seed=2 ** 63 + 5, tuple_scale=0.9, maximum_tuple_count=7)
    if name == "c600_cap1000":
        return src, tgt, corr, dict(seed=0, tuple_scale=0.95, maximum_tuple_count=1000)
    src, tgt, corr, _, _ = fc.case(1000, 0.8, 0)
    return src, tgt, corr, dict(seed=0, tuple_scale=0.95, maximum_tuple_count=1000)


@pytest.mark.parametrize("name", ["c60_cap7", "c600_cap1000", "limit"])
def test_tuples_equal_the_restatement_whatever_the_chunk(name):
    src, tgt, corr, kw = _tuples_case(name)
    p, q = _ref_pairs(src, tgt, corr)
    used, n_tuples, n_trials = of.tuples(p, q, kw["seed"], kw["tuple_scale"], kw["maximum_tuple_count"])
    if name == "limit":     # the trial limit ends the search: the last chunk is a partial one or a full one
        assert n_trials == 100 * corr.shape[0] and n_tuples < kw["maximum_tuple_count"]
        chunks = [0, 4096, 25000]
    else:                   # the cap falls on a chunk's last trial (whole, and the third of three), and strictly inside one
        assert n_tuples == kw["maximum_tuple_count"] and n_trials < 100 * corr.shape[0]
        third = n_trials // 3 if n_trials % 3 == 0 else n_trials
        inside = 64 if n_trials % 64 else 63
        chunks = [n_trials, third, inside, 0]
        assert n_trials % inside != 0
    plan, _ = _plan(src, tgt, corr)
    try:
        seen = []
        for chunk in chunks:
            plan.set_chunk(chunk)
            got = plan.tuples(**kw)
            assert got[0].dtype == np.int32 and got[0].tobytes() == used.tobytes(), chunk
            assert got[1:] == (n_tuples, n_trials), chunk
            seen.append(got[0].tobytes())
        assert len(set(seen)) == 1 and plan.used().tobytes() == used.tobytes()
    finally:
        plan.close()


def test_a_target_of_twice_the_size_passes_no_trial():
    src, tgt, corr, _, _ = fc.exact_case()
    gr = _gr()
    plan, (mean_p, mean_q, _) = _plan(src, 2.0 * tgt, corr)
    try:
        used, n_tuples, n_trials = plan.tuples()
        assert used.shape == (0,) and n_tuples == 0 and n_trials == 100 * corr.shape[0]
        plan.set_state()
        st = plan.iterate(64)
        assert st.status == "too_few" and st.n_iter == 0 and st.pose.tobytes() == of.IDENTITY.tobytes() and st.mu == 1.0
        assert plan.weights().shape == (0,)
    finally:
        plan.close()
    res = gr.registration_fgr(src, 2.0 * tgt, corr)
    assert res.status == "too_few" and res.n_tuples == 0 and res.n_iter == 0 and res.used.shape == (0,)
    ref = of.fgr(src, 2.0 * tgt, corr)
    assert ref["status"] == of.TOO_FEW
    assert np.array_equal(res.transformation.rot, np.eye(3)) and res.transformation.t.tobytes() == ref["t"].tobytes()


# ---------------------------------------------------------------------------------------------------------------- sums
@pytest.mark.parametrize("k", [1, 63, 64, 65, 3000, 4097])
def test_sums_equal_the_restatement_to_the_last_bit(k):
    p, q, pose, mu = fc.pair_cloud(max(k, 3))
    corr = np.stack([np.arange(p.shape[0]), np.arange(p.shape[0])], axis=1).astype(np.int32)
    rp, rq = _ref_pairs(p, q, corr)
    ref = of.sums(rp[:k], rq[:k], pose, mu)
    plan, _ = _plan(p, q, corr)
    try:
        plan.set_used(np.arange(k, dtype=np.int32))
        got = plan.sums(pose, mu)
        again = plan.sums()
        w = plan.weights()
        assert plan.state().objective == ref[27]
    finally:
        plan.close()
    assert got.shape == (28,) and got.tobytes() == ref.tobytes() and again.tobytes() == ref.tobytes()
    assert w.tobytes() == of.weights(rp[:k], rq[:k], pose, mu).tobytes()


# ---------------------------------------------------------------------------------------------------------------- step
def test_step_from_the_restatements_sums():
    p, q, pose, mu = fc.pair_cloud(300)
    corr = np.stack([np.arange(300), np.arange(300)], axis=1).astype(np.int32)
    rp, rq = _ref_pairs(p, q, corr)
    ref = of.sums(rp, rq, pose, mu)
    new, status, dis = of.step(pose, ref, 300)
    assert status == of.OK
    plan, _ = _plan(p, q, corr)
    try:
        plan.set_used(np.arange(300, dtype=np.int32))
        assert plan.sums(pose, mu).tobytes() == ref.tobytes()
        after = plan.step(decrease_mu=True, division_factor=1.4, maximum_correspondence_distance=0.025)
        st = plan.state()
    finally:
        plan.close()
    diff = float(np.max(np.abs(after - new)))
    print("host solves disagree by %.3e, GPU differs from the restatement by %.3e" % (dis, diff))
    assert diff <= of.step_bound(dis)
    assert st.status == "ok" and st.n_iter == 1 and st.mu == of.next_mu(mu, 0)


def test_collinear_pairs_are_degenerate_and_leave_the_pose():
    p = np.outer(np.linspace(-1.0, 1.0, 40), [1.0, 2.0, -0.5]) + np.array([0.1, 0.2, 0.3])
    corr = np.stack([np.arange(40), np.arange(40)], axis=1).astype(np.int32)
    rp, rq = _ref_pairs(p, p.copy(), corr)
    start = of.compose(of.delta_from_x(np.array([1.0e-3, -2.0e-3, 1.5e-3, 1.0e-3, 0.0, -1.0e-3])), of.IDENTITY)
    assert of.step(start, of.sums(rp, rq, start, 1.0), 40)[1] == of.DEGENERATE
    plan, _ = _plan(p, p.copy(), corr)
    try:
        plan.set_used(np.arange(40, dtype=np.int32))
        plan.set_state(start, 1.0)
        st = plan.iterate(64)
        assert st.status == "degenerate" and st.n_iter == 0 and st.mu == 1.0 and st.pose.tobytes() == start.tobytes()
    finally:
        plan.close()
    res = _gr().registration_fgr(p, p.copy(), corr, tuple_test=False)
    assert res.status == "degenerate" and res.n_iter == 0


# ---------------------------------------------------------------------------------------------------------------- loop
LOOP_CASES = [fc.LOOP["wrong50"] + (True,), fc.LOOP["wrong70"] + (True,), fc.LOOP["wrong80"] + (True,), (800, 0.7, 1, False)]


@pytest.mark.parametrize("c,wrong,seed,tuple_test", LOOP_CASES)
def test_loop_equals_the_restatement(c, wrong, seed, tuple_test):
    """64 iterations.  mu after every step and the step count are equal.  sin, cos and sqrt differ in the last place between
    the device and NumPy, so the pose and the weights are not byte-equal; they get 16 x the largest difference between the
    restatement as it is and the restatement with every pose entry moved by one ulp (up or down, seeded) after each step.
    Measured on the four cases with three seeds of the perturbation: the restatement moves by 6.7e-16 .. 2.6e-15 in the
    pose and by 1.4e-15 .. 6.1e-15 in the weights, so the bounds are 1.1e-14 .. 4.1e-14 and 2.3e-14 .. 9.8e-14."""
    src, tgt, corr, rot, t = fc.case(c, wrong, seed)
    ref = fc.reference(c, wrong, seed, tuple_test)
    per = of.fgr(src, tgt, corr, tuple_test=tuple_test, seed=seed, perturb=np.random.default_rng(0))
    pose_bound = 16.0 * float(np.max(np.abs(per["pose"] - ref["pose"])))
    weight_bound = 16.0 * float(np.max(np.abs(per["weights"] - ref["weights"])))
    assert per["mus"].tobytes() == ref["mus"].tobytes() and pose_bound > 0.0 and weight_bound > 0.0
    plan, _ = _plan(src, tgt, corr)
    try:
        if tuple_test:
            used, n_tuples, n_trials = plan.tuples(seed)
            assert used.tobytes() == ref["used"].tobytes() and (n_tuples, n_trials) == (ref["n_tuples"], ref["n_trials"])
        else:
            plan.set_used(np.arange(c, dtype=np.int32))
        plan.set_state(of.IDENTITY, 1.0)
        st = plan.iterate(64)
        w = plan.weights()
        plan.set_state(of.IDENTITY, 1.0)   # the same loop one step at a time: mu after every step, and the same bytes
        mus = [plan.iterate(1).mu for _ in range(64)]
        single = plan.state()
    finally:
        plan.close()
    d_pose, d_w = float(np.max(np.abs(st.pose - ref["pose"]))), float(np.max(np.abs(w - ref["weights"])))
    print("C = %d, %.0f %% wrong, tuple test %s: pose differs by %.3e (bound %.3e), weights by %.3e (bound %.3e)"
          % (c, 100 * wrong, tuple_test, d_pose, pose_bound, d_w, weight_bound))
    assert st.n_iter == ref["n_iter"] == 64 and st.status == "ok"
    assert np.array(mus).tobytes() == ref["mus"].tobytes() and st.mu == ref["mu"]
    assert single.pose.tobytes() == st.pose.tobytes() and single.n_iter == 64
    assert d_pose <= pose_bound and d_w <= weight_bound
    assert abs(st.objective - ref["objective"]) <= 1.0e-9 * max(1.0, ref["objective"])
    res = _gr().registration_fgr(src, tgt, corr, tuple_test=tuple_test, seed=seed)
    err = max(float(np.max(np.abs(res.transformation.rot - ref["rot"]))), float(np.max(np.abs(res.transformation.t - ref["t"]))))
    lever = 1.0 + ref["scale"] + float(np.max(np.abs(ref["mean_p"])))   # t_out = scale t + mean_q - R mean_p
    assert err <= pose_bound * 3.0 * lever and res.weights.tobytes() == w.tobytes() and res.mu == ref["mu"]
    assert res.used.tobytes() == ref["used"].tobytes() and (res.n_tuples, res.n_trials) == (ref["n_tuples"], ref["n_trials"])
    deg, shift = og.pose_error(res.transformation.rot, res.transformation.t, rot, t)
    assert deg <= fc.QUALITY_DEG and shift <= fc.QUALITY_SHIFT


# --------------------------------------------------------------------------------------------------------- whole calls
@pytest.fixture(scope="module")
def family_f():
    from probreg_amd import fpfh

    src, tgt, rot, t = og.family_f_clouds(1)
    feature_fn = fpfh.FPFH(*og.F_RADII)
    pairs, _ = _gr().feature_matching(feature_fn(src), feature_fn(tgt), mutual=True)
    return src, tgt, rot, t, feature_fn, pairs


def test_whole_calls_on_the_turned_surface(family_f):
    from probreg_amd import cpd

    src, tgt, rot, t, feature_fn, pairs = family_f
    gr = _gr()
    res = gr.registration_fgr(src, tgt, pairs, max_distance=og.F_TAU)
    glob = gr.registration_global(src, tgt, feature_fn=feature_fn, max_distance=og.F_TAU, method="fgr")
    assert isinstance(glob, gr.GlobalResult) and len(glob) == 4
    assert glob.transformation.rot.tobytes() == res.transformation.rot.tobytes()
    assert glob.transformation.t.tobytes() == res.transformation.t.tobytes()
    assert glob.fitness == res.fitness and glob.inlier_rmse == res.inlier_rmse and np.array_equal(glob.inliers, res.inliers)
    pose = np.concatenate([res.transformation.rot.reshape(9), res.transformation.t])
    plan = gr.RansacPlan()
    try:
        plan.set_correspondences(src[pairs[:, 0]], tgt[pairs[:, 1]])
        _, cnt, sm, inl = plan.refine(pose, og.F_TAU, 0)
    finally:
        plan.close()
    assert np.array_equal(res.inliers, np.nonzero(inl)[0]) and res.fitness == cnt / float(pairs.shape[0])
    assert res.inlier_rmse == (float(np.sqrt(sm / cnt)) if cnt else 0.0)
    deg, shift = og.pose_error(res.transformation.rot, res.transformation.t, rot, t)
    print("C = %d, %d tuples in %d trials, status %s: %.3f deg, %.4f, fitness %.3f" % (pairs.shape[0], res.n_tuples, res.n_trials,
                                                                                     res.status, deg, shift, res.fitness))
    assert res.status == "ok" and res.transformation.scale == 1.0
    kw = dict(maxiter=200, tol=1.0e-9, update_scale=False)
    got = cpd.registration_cpd(src, tgt, "rigid", tf_init_params=dict(rot=res.transformation.rot, t=res.transformation.t), **kw)
    want = cpd.registration_cpd(src, tgt, "rigid", tf_init_params=dict(rot=rot, t=t), **kw)
    d_rot = float(np.max(np.abs(got.transformation.rot - want.transformation.rot)))
    d_t = float(np.max(np.abs(got.transformation.t - want.transformation.t)))
    print("  CPD from the FGR pose against CPD from the ground truth: d_rot = %.2e, d_t = %.2e" % (d_rot, d_t))
    assert d_rot < 1.0e-4 and d_t < 1.0e-4


def test_method_ransac_returns_what_it_returns_today(family_f):
    src, tgt, _, _, feature_fn, pairs = family_f
    gr = _gr()
    kw = dict(n_hypotheses=4096, seed=og.F_SEED)
    direct = gr.registration_ransac(src, tgt, pairs, og.F_TAU, **kw)
    for extra in (dict(), dict(method="ransac")):
        res = gr.registration_global(src, tgt, feature_fn=feature_fn, max_distance=og.F_TAU, **kw, **extra)
        assert isinstance(res, gr.GlobalResult)
        assert res.transformation.rot.tobytes() == direct.transformation.rot.tobytes()
        assert res.transformation.t.tobytes() == direct.transformation.t.tobytes()
        assert res.fitness == direct.fitness and res.inlier_rmse == direct.inlier_rmse
        assert res.inliers.tobytes() == direct.inliers.tobytes()


# --------------------------------------------------------------------------------------------------------------- reuse
def _run(plan, src, tgt, corr, seed):
    plan.set_clouds(src, tgt)
    plan.set_correspondences(corr)
    norm = plan.normalise()
    used, n_tuples, n_trials = plan.tuples(seed)
    plan.set_state(of.IDENTITY, 1.0)
    st = plan.iterate(64)
    return (norm[0].tobytes(), norm[1].tobytes(), norm[2], used.tobytes(), n_tuples, n_trials, st.pose.tobytes(), st.mu, st.n_iter,
            st.status, plan.weights().tobytes(), plan.state(caller_units=True).pose.tobytes())


def test_one_plan_run_twice_gives_what_two_fresh_plans_give():
    big = fc.case(800, 0.7, 1)[:3]
    small = (big[0][:700], big[1][:900], fc.case(600, 0.5, 0)[2][:70] % 700)
    gr = _gr()
    fresh = []
    for src, tgt, corr in (big, small, big):
        plan = gr.FgrPlan()
        try:
            fresh.append(_run(plan, src, tgt, corr, 3))
        finally:
            plan.close()
    plan = gr.FgrPlan()
    try:
        reused = [_run(plan, src, tgt, corr, 3) for src, tgt, corr in (big, small, big)]
    finally:
        plan.close()
    assert reused == fresh and fresh[0] == fresh[2] and fresh[0] != fresh[1]
