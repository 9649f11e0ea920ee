"""Global registration on the GPU (probreg_amd.global_reg, csrc/global_reg.hip) against its restatement
(tests/oracle_global_reg.py), stage by stage and end to end.

Discrete results (match indices, triples, validity flags, inlier counts, winners, inlier sets) are compared exactly: the CPU
tests (test_oracle_global_reg.py) show that no decision of these cases lies within 1e-9 (relative) of its threshold.  D^2 is
compared to the last bit.  Poses of three-point solves get 8 x the disagreement of two independent host solves (NumPy SVD,
Horn's quaternions) on the same triples, or 1e-12 where that is larger; ordered sums get C 2^-52 relative.
"""
import numpy as np
import pytest

import oracle_global_reg as og

pytestmark = pytest.mark.gpu


def _gr():
    from probreg_amd import global_reg
    return global_reg


def _features(na, nb, d, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (na, d)), rng.uniform(0.0, 1.0, (nb, d))


# ------------------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize("na,nb,d,segments", [(1, 1, 1, 0), (1, 70, 33, 0), (65, 63, 33, 0), (257, 1000, 64, 0),
                                              (257, 1000, 64, 7), (300, 5, 33, 64), (70, 300, 9, 3), (40, 50, 40, 0)])
def test_matching_equals_the_restatement_to_the_last_bit(na, nb, d, segments):
    a, b = _features(na, nb, d, 100 + na + nb + d)
    idx, d2 = _gr().nearest_feature(a, b, segments=segments)
    ref_idx, ref_d2 = og.match(a, b)
    assert idx.dtype == np.int32 and np.array_equal(idx, ref_idx)
    assert np.array_equal(d2, ref_d2)


def test_matching_family_s_mutual_filter_and_second_run():
    f = og.family_s(1)
    gr = _gr()
    idx, d2 = gr.nearest_feature(f["source_feature"], f["target_feature"])
    ref_idx, ref_d2 = og.match(f["source_feature"], f["target_feature"])
    assert np.array_equal(idx, ref_idx) and np.array_equal(d2, ref_d2)
    pairs, pd2 = gr.feature_matching(f["source_feature"], f["target_feature"], mutual=True)
    assert pairs.dtype == np.int32 and np.array_equal(pairs, f["pairs"]) and np.array_equal(pd2, f["d2"])
    again, ad2 = gr.feature_matching(f["source_feature"], f["target_feature"], mutual=True)
    assert pairs.tobytes() == again.tobytes() and pd2.tobytes() == ad2.tobytes()
    every, _ = gr.feature_matching(f["source_feature"], f["target_feature"], mutual=False)
    assert np.array_equal(every[:, 0], np.arange(1500)) and np.array_equal(every[:, 1], ref_idx)


def test_matching_ties_go_to_the_smaller_index():
    a, b = _features(130, 300, 33, 5)
    b[240] = b[7]
    b[23] = b[7]
    b[299] = b[150]
    a[0] = b[7] + 1.0e-3
    a[5] = b[7]
    a[129] = b[150]
    for segments in (0, 1, 2, 300):  # the duplicates fall into one segment, into two, and each row is a segment
        idx, d2 = _gr().nearest_feature(a, b, segments=segments)
        assert idx[0] == 7 and idx[5] == 7 and idx[129] == 150 and d2[5] == 0.0
        assert np.array_equal(idx, og.match(a, b)[0])
    pairs, _ = _gr().feature_matching(a, b, mutual=True)
    assert np.array_equal(pairs, og.feature_matching(a, b, True)[0])


# --------------------------------------------------------------------------------------------------------------- build
@pytest.mark.parametrize("c", og.BUILD_C)
@pytest.mark.parametrize("n_hyp", og.BUILD_H)
def test_build_equals_the_restatement(c, n_hyp):
    p, q = og.corr_case(c)
    ref = og.build_case(c, n_hyp)
    bound = og.solve_bound(og.solver_disagreement(p, q, ref))
    plan = _gr().RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.build(og.CASE_SEED, n_hyp)
        tri, pose, valid = plan.hypotheses()
    finally:
        plan.close()
    assert np.array_equal(tri, ref["triples"])
    assert np.array_equal(valid, ref["valid"])
    assert np.all(pose[~valid] == 0.0)
    err = float(np.max(np.abs(pose[valid] - ref["pose"][valid]))) if valid.any() else 0.0
    det = np.linalg.det(pose[valid, :9].reshape(-1, 3, 3)) if valid.any() else np.ones(1)
    print("build C = %d, H = %d: valid = %d, pose err = %.3e (bound %.3e), |det - 1| = %.3e"
          % (c, n_hyp, int(valid.sum()), err, bound, float(np.max(np.abs(det - 1.0)))))
    assert err <= bound
    assert np.max(np.abs(det - 1.0)) <= bound


def test_build_in_two_pieces_gives_what_one_call_gives():
    p, q = og.corr_case(427)
    plan = _gr().RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.build(og.CASE_SEED, 4096)
        whole = plan.hypotheses()
        plan.build(og.CASE_SEED, 1000, offset=0)
        head = plan.hypotheses()
        plan.build(og.CASE_SEED, 3096, offset=1000)
        tail = plan.hypotheses()
    finally:
        plan.close()
    for w, h, t in zip(whole, head, tail):
        assert w.tobytes() == np.concatenate([h, t]).tobytes()


# ------------------------------------------------------------------------------------------------------------- scoring
@pytest.mark.parametrize("c", og.SCORE_C)
@pytest.mark.parametrize("n_hyp", og.SCORE_H)
def test_scoring_on_explicit_hypotheses(c, n_hyp):
    p, q = og.corr_case(c)
    pose, valid, ref_count, ref_sum, band, ref_win = og.score_case(c, n_hyp)
    assert band == 0
    plan = _gr().RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.set_hypotheses(pose, valid)
        plan.score(og.CASE_TAU)
        count, total = plan.scores()
        win, wcount, wsum, wpose = plan.best()
    finally:
        plan.close()
    assert np.array_equal(count, ref_count)
    assert np.all(total[~valid] == 0.0)
    assert np.all(np.abs(total - ref_sum) <= c * 2.0 ** -52 * np.abs(ref_sum))
    assert win == ref_win and wcount == ref_count[ref_win] and wsum == total[win]
    assert np.array_equal(wpose, pose[win])


def test_scoring_more_than_one_segment_and_more_than_one_batch():
    """C past the 1024 correspondences of a segment, more valid hypotheses than the 65536 of a launch; a sample is compared."""
    rng = np.random.default_rng(77)
    c, n_hyp = 2500, 100000  # two thirds are valid: the 65536th valid one is hypothesis 98304
    p = rng.uniform(-1.0, 1.0, (c, 3))
    q = p @ og.ROT_S.T + og.SHIFT + rng.normal(0.0, 0.01, (c, 3))
    pose = np.tile(np.concatenate([og.ROT_S.reshape(9), og.SHIFT]), (n_hyp, 1))
    pose[:, 9:] += rng.normal(0.0, 0.01, (n_hyp, 3))
    valid = np.ones(n_hyp, dtype=bool)
    valid[::3] = False
    sample = np.concatenate([np.arange(1, 40), np.arange(98200, 98400), np.arange(n_hyp - 30, n_hyp)])
    mask = np.zeros(n_hyp, dtype=bool)
    mask[sample] = True
    ref_count, ref_sum, band = og.score(p, q, pose, valid & mask, og.CASE_TAU)
    assert band == 0
    plan = _gr().RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.set_hypotheses(pose, valid)
        plan.score(og.CASE_TAU)
        count, total = plan.scores()
        plan.score(og.CASE_TAU)
        count2, total2 = plan.scores()
    finally:
        plan.close()
    sel = sample[valid[sample]]
    assert np.array_equal(count[sel], ref_count[sel])
    assert np.all(np.abs(total[sel] - ref_sum[sel]) <= c * 2.0 ** -52 * np.abs(ref_sum[sel]))
    assert np.all(count[~valid] == -1) and np.all(count[valid] >= 0)
    assert count.tobytes() == count2.tobytes() and total.tobytes() == total2.tobytes()


def test_equal_scores_go_to_the_smaller_hypothesis():
    p, q = og.corr_case(65)
    pose, valid, _, _, _, _ = og.score_case(65, 63)
    pose = pose.copy()
    # the least-squares pose of the true pairs, three times: it has every true pair as an inlier and the smallest sum
    true = og.residuals2(p, q, np.concatenate([og.ROT_S.reshape(9), og.SHIFT]))[0] <= og.CASE_TAU ** 2
    rot, t = og.kabsch_svd(p[true], q[true])
    pose[9] = pose[5] = pose[40] = np.concatenate([rot.reshape(9), t])
    ref_count, ref_sum, band = og.score(p, q, pose, np.ones(63, dtype=bool), og.CASE_TAU)
    assert band == 0 and og.winner(ref_count, ref_sum) == 5
    plan = _gr().RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.set_hypotheses(pose, np.ones(63, dtype=bool))
        plan.score(og.CASE_TAU)
        count, total = plan.scores()
        win = plan.best()[0]
    finally:
        plan.close()
    assert np.array_equal(count, ref_count)
    assert count[5] == count[9] == count[40] and total[5] == total[9] == total[40]
    assert win == 5


def test_no_valid_hypothesis_is_an_error():
    from probreg_amd import _lib

    p, q = og.corr_case(65)
    pose, valid, _, _, _, _ = og.score_case(65, 63)
    plan = _gr().RansacPlan()
    try:
        plan.set_correspondences(p, q)
        plan.set_hypotheses(pose, np.zeros(63, dtype=bool))
        plan.score(og.CASE_TAU)
        count, _ = plan.scores()
        assert np.all(count == -1)
        with pytest.raises(_lib.ProbregHipError, match="valid"):
            plan.best()
    finally:
        plan.close()
    # through the public call: three correspondences on a line never give a valid triangle
    line = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    with pytest.raises(_lib.ProbregHipError, match="valid"):
        _gr().registration_ransac(line, line, np.array([[0, 0], [1, 1], [2, 2]]), 0.1, n_hypotheses=256)


def test_abi_argument_errors_on_a_handle():
    import ctypes

    from probreg_amd import _lib

    p, q = og.corr_case(65)
    plan = _gr().RansacPlan()
    try:
        h = plan._h
        assert _lib.lib.prg_ransac_set_correspondences(h, _lib.ptr(p), _lib.ptr(q), 2) == _lib.PRG_ERR_INVALID
        assert "C" in _lib.last_error()
        assert _lib.lib.prg_ransac_build(h, 0, 0, 16, 0.9) == _lib.PRG_ERR_STATE
        plan.set_correspondences(p, q)
        assert _lib.lib.prg_ransac_build(h, 0, 0, 0, 0.9) == _lib.PRG_ERR_INVALID
        assert "H" in _lib.last_error()
        assert _lib.lib.prg_ransac_build(h, 0, 0, 16, 1.5) == _lib.PRG_ERR_INVALID
        assert _lib.lib.prg_ransac_score(h, 0.1) == _lib.PRG_ERR_STATE
        plan.build(0, 16)
        for tau in (float("nan"), float("inf"), -1.0):
            assert _lib.lib.prg_ransac_score(h, tau) == _lib.PRG_ERR_INVALID
            assert "tau" in _lib.last_error()
            pose = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
            assert _lib.lib.prg_ransac_refine(h, tau, 1, _lib.ptr(pose), None, None, None) == _lib.PRG_ERR_INVALID
        assert _lib.lib.prg_ransac_get_scores(h, None, None) == _lib.PRG_ERR_STATE
        cnt = ctypes.c_int(0)
        assert _lib.lib.prg_ransac_best(h, None, ctypes.byref(cnt), None, None) == _lib.PRG_ERR_STATE
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------------- end to end
def _pose_bound(p, q, ref):
    """The solve bound of the last refit (8 x SVD-against-Horn on the inliers it ran on, or 1e-12) times that refit's
    condition max(1, s1 / (s2 + s3)).  The refits before it enter through their inlier sets only, and those are equal."""
    return og.solve_bound(og.refit_disagreement(p, q, ref["fitted"])) * og.refit_condition(p, q, ref["fitted"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_end_to_end_family_s(seed):
    f = og.family_s(seed)
    ref = og.family_s_ransac(seed)
    assert ref["band"] == 0
    gr = _gr()
    pairs, _ = gr.feature_matching(f["source_feature"], f["target_feature"], mutual=True)
    assert np.array_equal(pairs, f["pairs"])
    res = gr.registration_ransac(f["source"], f["target"], pairs, og.S_TAU, n_hypotheses=og.S_HYP, seed=og.S_SEED)
    assert np.array_equal(res.inliers, ref["inliers"])
    assert res.fitness == ref["fitness"]
    assert abs(res.inlier_rmse - ref["inlier_rmse"]) <= 1e-12 + pairs.shape[0] * 2.0 ** -52 * ref["inlier_rmse"]
    bound = _pose_bound(f["p"], f["q"], ref)
    err = max(float(np.max(np.abs(res.transformation.rot - ref["rot"]))), float(np.max(np.abs(res.transformation.t - ref["t"]))))
    print("family S seed %d: pose err = %.3e (bound %.3e)" % (seed, err, bound))
    assert err <= bound and res.transformation.scale == 1.0
    rot_err, t_err = og.pose_error(res.transformation.rot, res.transformation.t, f["rot"], f["t"])
    assert rot_err < 0.1 and t_err < 2.0e-3
    # the stages on a plan: the same winner, and the same scores when the hypotheses are built and scored in two pieces
    plan = gr.RansacPlan()
    try:
        plan.set_correspondences(f["p"], f["q"])
        plan.build(og.S_SEED, og.S_HYP)
        plan.score(og.S_TAU)
        count, total = plan.scores()
        win, wcount, _, wpose = plan.best()
        pose, cnt, sm, inl = plan.refine(wpose, og.S_TAU, 3)
        pieces = []
        for off, n in ((0, 1500), (1500, og.S_HYP - 1500)):
            plan.build(og.S_SEED, n, offset=off)
            plan.score(og.S_TAU)
            pieces.append(plan.scores())
    finally:
        plan.close()
    assert win == ref["winner"] and wcount == ref["count"][win]
    assert np.array_equal(count, ref["count"])
    assert count.tobytes() == np.concatenate([pieces[0][0], pieces[1][0]]).tobytes()
    assert total.tobytes() == np.concatenate([pieces[0][1], pieces[1][1]]).tobytes()
    assert np.array_equal(np.nonzero(inl)[0], ref["inliers"]) and cnt == ref["final_count"]
    assert np.array_equal(pose[:9].reshape(3, 3), res.transformation.rot) and np.array_equal(pose[9:], res.transformation.t)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_end_to_end_family_f_and_a_local_method_started_from_it(seed):
    from probreg_amd import cpd, fpfh

    src, tgt, rot, t = og.family_f_clouds(seed)
    gr = _gr()
    feature_fn = fpfh.FPFH(*og.F_RADII)
    res = gr.registration_global(src, tgt, feature_fn=feature_fn, max_distance=og.F_TAU, n_hypotheses=og.F_HYP, seed=og.F_SEED)
    # the restatement on the same descriptors
    pairs, _ = og.feature_matching(feature_fn(src), feature_fn(tgt), mutual=True)
    p, q = src[pairs[:, 0]], tgt[pairs[:, 1]]
    ref = og.ransac(p, q, og.F_TAU, og.F_HYP, og.F_SEED)
    assert ref["band"] == 0
    assert np.array_equal(res.inliers, ref["inliers"]) and res.fitness == ref["fitness"]
    bound = _pose_bound(p, q, ref)
    err = max(float(np.max(np.abs(res.transformation.rot - ref["rot"]))), float(np.max(np.abs(res.transformation.t - ref["t"]))))
    rot_err, t_err = og.pose_error(res.transformation.rot, res.transformation.t, rot, t)
    print("family F seed %d: C = %d, pose err = %.3e (bound %.3e), rot_err = %.3f deg, t_err = %.4f"
          % (seed, pairs.shape[0], err, bound, rot_err, t_err))
    assert err <= bound
    assert rot_err < 6.0 and t_err < 0.05
    # a rigid CPD started from it ends where the same call started from the ground truth ends
    kw = dict(maxiter=200, tol=1.0e-9, update_scale=False)  # both stop on tol (the NumPy oracle: after 77 to 81 iterations)
    got = cpd.registration_cpd(src, tgt, "rigid", tf_init_params=dict(rot=res.transformation.rot, t=res.transformation.t), **kw)
    want = cpd.registration_cpd(src, tgt, "rigid", tf_init_params=dict(rot=rot, t=t), **kw)
    d_rot = float(np.max(np.abs(got.transformation.rot - want.transformation.rot)))
    d_t = float(np.max(np.abs(got.transformation.t - want.transformation.t)))
    print("  CPD from the global pose against CPD from the ground truth: d_rot = %.2e, d_t = %.2e" % (d_rot, d_t))
    assert d_rot < 1.0e-4 and d_t < 1.0e-4
