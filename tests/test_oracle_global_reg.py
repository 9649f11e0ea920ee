"""The restatement of global registration (tests/oracle_global_reg.py) on its own: pinned draws, the
tie rule, pose recovery on both test families, and the band condition that lets the GPU tests ask for exact discrete results.
No GPU."""
import numpy as np
import pytest

import oracle_global_reg as og


def test_pinned_draws():
    assert og.draw(7, [0, 1, 2, 3], 1000).tolist() == [[389, 16, 900], [582, 452, 249], [467, 328, 134], [413, 103, 959]]
    assert og.draw(0, [0, 1048575], 100000).tolist() == [[88331, 43152, 2643], [98746, 11942, 67702]]


def test_draws_do_not_depend_on_how_the_range_is_cut():
    whole = og.build(*og.corr_case(64), og.CASE_SEED, 100)
    tail = og.build(*og.corr_case(64), og.CASE_SEED, 60, h_offset=40)
    assert np.array_equal(whole["triples"][40:], tail["triples"]) and np.array_equal(whole["valid"][40:], tail["valid"])
    assert np.array_equal(whole["pose"][40:], tail["pose"])


def test_ties_go_to_the_smaller_index():
    rng = np.random.default_rng(3)
    b = rng.uniform(0.0, 1.0, (50, 33))
    b[40] = b[7]
    b[23] = b[7]
    a = rng.uniform(0.0, 1.0, (20, 33))
    a[0] = b[7] + 1.0e-3
    a[5] = b[7]
    idx, d2 = og.match(a, b)
    assert idx[0] == 7 and idx[5] == 7 and d2[5] == 0.0
    # D^2 is the k-loop of the definition to the last bit
    acc = 0.0
    for k in range(33):
        diff = a[0, k] - b[7, k]
        acc = acc + diff * diff
    assert d2[0] == acc
    pairs, _ = og.feature_matching(a, b, mutual=True)
    assert np.all(np.diff(pairs[:, 0]) > 0)
    iba, _ = og.match(b, a)
    assert all(iba[t] == s for s, t in pairs)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_family_s_pose_is_recovered(seed):
    f = og.family_s(seed)
    r = og.family_s_ransac(seed)
    rot_err, t_err = og.pose_error(r["rot"], r["t"], f["rot"], f["t"])
    print("family S seed %d: C = %d, valid = %d, winner = %d, inliers = %d, rot_err = %.4f deg, t_err = %.2e, band = %d"
          % (seed, f["p"].shape[0], int(r["build"]["valid"].sum()), r["winner"], r["final_count"], rot_err, t_err, r["band"]))
    assert rot_err < 0.1 and t_err < 2.0e-3
    assert abs(np.linalg.det(r["rot"]) - 1.0) < 1e-12
    assert r["fitness"] == r["final_count"] / f["p"].shape[0] and r["inlier_rmse"] <= og.S_TAU
    assert r["band"] == 0  # the GPU's end-to-end test asks for the same winner and inlier set


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_family_f_pose_is_recovered(seed):
    import oracle_fpfh

    src, tgt, rot, t = og.family_f_clouds(seed)
    fa = oracle_fpfh.describe(src, *og.F_RADII)["fpfh"]
    fb = oracle_fpfh.describe(tgt, *og.F_RADII)["fpfh"]
    pairs, _ = og.feature_matching(fa, fb, mutual=True)
    r = og.ransac(src[pairs[:, 0]], tgt[pairs[:, 1]], og.F_TAU, og.F_HYP, og.F_SEED)
    rot_err, t_err = og.pose_error(r["rot"], r["t"], rot, t)
    print("family F seed %d: C = %d, valid = %d, inliers = %d, rot_err = %.3f deg, t_err = %.4f"
          % (seed, pairs.shape[0], int(r["build"]["valid"].sum()), r["final_count"], rot_err, t_err))
    assert rot_err < 6.0 and t_err < 0.05


@pytest.mark.parametrize("c", og.BUILD_C)
def test_band_condition_and_solver_yardstick_of_the_build_cases(c):
    """No validity check of a GPU build case lies within 1e-9 (relative) of its threshold; the disagreement of the two host
    solves, 8 x which (or 1e-12) the HIP path gets, is printed."""
    p, q = og.corr_case(c)
    for n_hyp in og.BUILD_H:
        b = og.build_case(c, n_hyp)
        assert int(np.count_nonzero(b["margin"] <= og.BAND)) == 0
        dis = og.solver_disagreement(p, q, b)
        print("build case C = %d, H = %d: valid = %d, SVD vs Horn = %.3e, HIP bound = %.3e"
              % (c, n_hyp, int(b["valid"].sum()), dis, og.solve_bound(dis)))
        assert dis < 1.0e-9  # two fp64 solves of a triple that passed the degeneracy check
    assert og.build_case(c, 4096)["valid"].any()


@pytest.mark.parametrize("c", og.SCORE_C)
def test_band_condition_of_the_scoring_cases(c):
    for n_hyp in og.SCORE_H:
        pose, valid, count, total, band, win = og.score_case(c, n_hyp)
        assert band == 0
        assert win >= 0 and valid[win]
        if n_hyp >= 63:  # residuals on both sides of tau, or the stage is not exercised
            assert count[valid].min() < c and count[valid].max() > 0


def test_winner_key():
    count = np.array([-1, 5, 7, 7, 7, -1])
    total = np.array([0.0, 0.1, 0.3, 0.2, 0.2, 0.0])
    assert og.winner(count, total) == 3
    assert og.winner(np.array([-1, -1]), np.zeros(2)) == -1


def test_refine_keeps_a_pose_without_three_inliers():
    p, q = og.corr_case(64)
    pose = np.concatenate([np.eye(3).reshape(9), [50.0, 50.0, 50.0]])
    out, cnt, sm, inl, _, fitted = og.refine(p, q, pose, og.CASE_TAU, 3)
    assert np.array_equal(out, pose) and cnt == 0 and sm == 0.0 and inl.shape == (0,) and fitted.shape == (0,)
