"""tests/oracle_gmmfit.py has to be right before the product is compared with it (no GPU): its EM iteration against
scikit-learn's recorded results, its seeding against plain loops without a cumulative sum, its Lloyd iterations
against counts derived by hand on an integer lattice, its M-step on labels against NumPy's mean and variance, and the
margins of the three stage cases that are exact by construction."""
import os

import numpy as np
import pytest

import oracle_gmmfit as og
from conftest import GOLDEN_DIR, Golden


@pytest.fixture(scope="module")
def golden():
    return Golden(os.path.join(GOLDEN_DIR, "gmmreg_golden.npz"))


def close(got, ref, sens, what):
    """The rule of tests/test_gmmreg_gpu.py: scikit-learn expands |x - mu|^2, so its result moves by ``sens`` when the
    data move by one ulp."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, what
    err = float(np.max(np.abs(got - ref))) / float(np.max(np.abs(ref)))
    bound = max(10.0 * float(sens), 1.0e-9)
    print("%s: err %.3e bound %.3e" % (what, err, bound))
    assert err <= bound, "%s: %.3e of its scale, bound %.3e" % (what, err, bound)


@pytest.mark.parametrize("name", ["bunny_k32", "fish_k32", "surface5k_k100", "surface5k_far"])
def test_em_step_matches_sklearn(golden, name):
    from probreg_amd import synthetic

    case = golden.case("em/" + name)
    spec = [str(s) for s in case["spec"]]
    if spec[0] == "surface":
        x = synthetic.surface(int(spec[1]), int(spec[2]))
        x = x - x.mean(axis=0)
    else:
        x = case["x"]
    k = int(case["k"])
    mu = x[case["init_idx"]].copy()
    mu[0] = case["init_mean0"]
    w, cov = np.full(k, 1.0 / k), np.full(k, 1.0 / float(case["init_precision"]))
    for it in (1, 2, 3):
        w, mu, cov, lb = og.em_step(x, w, mu, cov, 1.0e-6)
        close(lb, case["lower_bounds"][it - 1], case["sens_lower_bounds"], "%s lower bound %d" % (name, it))
        if "mi%d_means" % it in case:
            close(w, case["mi%d_weights" % it], case["sens_weights"], "%s weights after %d" % (name, it))
            close(mu, case["mi%d_means" % it], case["sens_means"], "%s means after %d" % (name, it))
            close(cov, case["mi%d_covariances" % it], case["sens_covariances"], "%s covariances after %d" % (name, it))
        if it == 1 and name == "surface5k_far":  # the component whose responsibilities underflow
            assert np.all(mu[0] == 0.0) and abs(cov[0] - 1.0e-6) < 1e-20 and 0.0 < w[0] < 1e-15


def test_seed_matches_brute_force():
    from probreg_amd import synthetic

    x = synthetic.surface(300, 40)
    k = 12
    u = np.random.RandomState(11).random_sample((k, 2 + int(np.log(k))))
    idx, margins = og.seed(x, k, u)
    bound = og.decision_bound(x.shape[0])
    print("winner margin %.3e sampling margin %.3e bound %.3e" % (margins["winner"].min(), margins["sampling"].min(),
                                                                  bound))
    assert margins["winner"].min() >= bound and margins["sampling"].min() >= bound
    assert idx[0] == min(int(u[0, 0] * 300), 299) and len(np.unique(idx)) == k
    assert idx.tolist() == og.seed_brute_force(x, k, u).tolist()
    # every point a centre already: the target is 0 and the first point is taken
    same = np.repeat(x[:1], 5, axis=0)
    idx, margins = og.seed(same, 3, u[:3], exact=True)
    assert idx.tolist() == [min(int(u[0, 0] * 5), 4), 0, 0] and np.all(np.isinf(margins["winner"]))


def lattice():
    return np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(4.0), indexing="ij"), axis=-1).reshape(-1, 3)


def test_lloyd_counts_on_a_lattice():
    """{0..3}^3 with centres at lattice points; every count below follows from the first-minimum rule by hand."""
    x = lattice()
    # (0,0,0) and (2,0,0): the plane x = 1 is equidistant and goes to the first centre, so the split is x <= 1 | x >= 2.
    # The means (0.5, 1.5, 1.5) and (2.5, 1.5, 1.5) split at x = 1.5: nothing changes in iteration 2.
    # (Ties towards the last minimum would give x = 0 | x >= 1, 16 and 48, and stay there.)
    c, n_iter, counts, m = og.lloyd(x, np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), 300, 0.0, exact=True)
    assert n_iter == 2 and counts.tolist() == [32, 32]
    assert c.tolist() == [[0.5, 1.5, 1.5], [2.5, 1.5, 1.5]]
    assert m["label_gap"] > 0.1 and m["labels"].tolist() == (x[:, 0] >= 2).astype(int).tolist()
    # without exact=True the same run reports the tie as a decision that rounding could turn
    assert og.lloyd(x, np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), 300, 0.0)[3]["label_gap"] == 0.0
    # one iteration only: the update has run once, the labels are those of the updated centres
    c, n_iter, counts, _ = og.lloyd(x, np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), 1, 0.0, exact=True)
    assert n_iter == 1 and counts.tolist() == [32, 32] and c.tolist() == [[0.5, 1.5, 1.5], [2.5, 1.5, 1.5]]
    # a copy of the second centre wins no tie in the first assignment: it is empty in the update and keeps its place
    c, n_iter, _, _ = og.lloyd(x, np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), 1, 0.0, exact=True)
    assert n_iter == 1 and c.tolist() == [[0.5, 1.5, 1.5], [2.5, 1.5, 1.5], [2.0, 0.0, 0.0]]
    # a centre no point is nearest to stays empty, stays where it is and adds nothing to the shift
    c, n_iter, counts, _ = og.lloyd(x, np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [9.0, 9.0, 9.0]]), 300, 0.0, exact=True)
    assert n_iter == 2 and counts.tolist() == [32, 32, 0] and c[2].tolist() == [9.0, 9.0, 9.0]
    # four centres on a square: x = 1 goes left, y = 1 goes down, (1, 1, z) is a four-way tie for the first centre
    sq = np.array([[0.0, 0.0, 0.0], [0.0, 2.0, 0.0], [2.0, 0.0, 0.0], [2.0, 2.0, 0.0]])
    c, n_iter, counts, _ = og.lloyd(x, sq, 300, 0.0, exact=True)
    assert n_iter == 2 and counts.tolist() == [16, 16, 16, 16]
    assert c.tolist() == [[0.5, 0.5, 1.5], [0.5, 2.5, 1.5], [2.5, 0.5, 1.5], [2.5, 2.5, 1.5]]
    # the shift test: the first update moves the two centres by 0.25 + 2.25 + 2.25 each, 9.5 in all
    assert og.lloyd(x, sq[[0, 2]], 300, 9.5, exact=True)[1] == 1
    _, n_iter, _, m = og.lloyd(x, sq[[0, 2]], 300, 9.0)
    assert n_iter == 2 and abs(m["stop"] - 0.5 / 9.0) < 1e-15


def test_init_from_labels_is_mean_and_variance():
    from probreg_amd import synthetic

    x = synthetic.surface(500, 41)
    labels = np.random.default_rng(5).integers(0, 7, 500)
    labels[labels == 3] = 2  # an empty component
    for data in (x, x[:, :2]):
        w, mu, cov = og.init_from_labels(data, labels, 7, 1.0e-6)
        for j in range(7):
            p = data[labels == j]
            if j == 3:
                assert w[j] == og.TEN_EPS / 500 and np.all(mu[j] == 0.0) and abs(cov[j] - 1.0e-6) < 1e-20
                continue
            assert abs(w[j] - p.shape[0] / 500.0) < 1e-15
            assert np.max(np.abs(mu[j] - p.mean(axis=0))) < 1e-13
            assert abs(cov[j] - (p.var(axis=0).mean() + 1.0e-6)) < 1e-13
    # the EM iteration from one-hot-like parameters far apart reproduces the same M-step
    far = np.concatenate([x[:100] * 1e-3, x[100:200] * 1e-3 + 50.0])
    lab = np.repeat([0, 1], 100)
    w, mu, cov = og.init_from_labels(far, lab, 2, 1.0e-6)
    w2, mu2, cov2, _ = og.em_step(far, w, mu, cov, 1.0e-6)
    assert np.max(np.abs(w2 - w)) < 1e-15 and np.max(np.abs(mu2 - mu)) < 1e-13 and np.max(np.abs(cov2 - cov)) < 1e-13


@pytest.mark.parametrize("name", ["one", "dup64", "lattice", "s257_k16"])
def test_stage_case_margins(name):
    """The decisions of the cases that are exact by construction (and of one ordinary case) are clear of rounding."""
    import test_gmmfit_stages_gpu as stages

    stages.seeding_is_clear(name)
    stages.lloyd_is_clear(name)
    if name == "lattice":
        stages.lloyd_is_clear(name, 1)
    if name == "dup64":
        idx, _ = stages.oracle_seed(name)
        x = stages.make_case(name)["x"]
        assert len(np.unique(x[idx], axis=0)) == 32 and np.all(idx[33:] == 0)  # the zero-potential fallback
