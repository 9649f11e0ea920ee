"""The mixture fit of csrc/gmmfit.hip stage by stage against tests/oracle_gmmfit.py: the k-means++ seeds, the Lloyd
iterations, the M-step on the labels and single EM iterations, at the shapes where the kernels change path.

Cases (cloud, K, random_state of ``features.seed_uniforms``) and what each reaches:
  s5000_k100    surface(5000, 31), 100, 3          ragged last seed chunk, 6 trials
  s257_k16      surface(257, 32), 16, 4            one full seed chunk + 1 point
  s262444_k8    surface(262444, 33), 8, 5          1026 seed chunks: two per thread of k_seed_choose; moment chunks of 640
  s131201_k5    surface(131201, 36), 5, 8          moment chunks of 384, the last one 257 points = LDS tiles 128, 128, 1
  d2_1000_k20   surface(1000, 34)[:, :2], 20, 6    dim = 2 (padded to 3 on the device)
  far_3000_k32  surface(3000, 35) + offset, 32, 7  a cloud far from the origin
  s1000_k129    surface(1000, 37), 129, 9          the second block of 128 components holds one component
  one           one point, 1, 0                    N = K = 1
  dup64         surface(32, 38) twice, 64, 2       K = N with bitwise duplicates: zero total potential, duplicate centres,
                                                   empty clusters (random_state 1 failed the winner margin: two candidates
                                                   tie in exact arithmetic, their potentials differ by rounding alone)
  lattice       {0..3}^3 shuffled, 8, 2            integer coordinates: exact ties, broken by the first-minimum rule

Conditions.  Seeds, iteration counts and label counts are compared exactly, so every test first asserts on the oracle's
margins alone that no decision behind them is a matter of rounding: winner and sampling margins of the seeding, the
label gap of every Lloyd assignment (divided by max(1, max|x| / d), d the nearest distance) and the distance of every
summed shift from the tolerance (same rule with d = sqrt(tol)) are at least 16 N eps.  N eps bounds the relative error
of an N-term fp64 sum of same-signed terms in any order; candidates are data points, centres are means of up to N
coordinates of size max|x|.  ``dup64``, ``lattice`` and ``one`` are exact by construction for the ties they are built
to contain (oracle_gmmfit's ``exact=True``); every other decision of theirs meets the same bound.

Tolerances of the real-valued outputs.  Both sides evaluate the same formula and differ in summation order and in the
last bits of exp / log / sqrt: 16 N eps of the quantity's scale (max |value| for weights and the lower bound, max|x|
for centres and means), and 16 N eps max|x|^2 for covariances, which subtract mean^2 from a second moment.  An EM
iteration is compared from identical fp64 parameters on both sides (the product's own M-step on the labels, then the
oracle's first result), so that an earlier stage's rounding, which cov = E x^2 - mean^2 amplifies, is not charged to it.
"""
import functools

import numpy as np
import pytest

import oracle_gmmfit as og

pytestmark = pytest.mark.gpu

REG_COVAR = 1.0e-6
#        name           K   rs  exact  Lloyd iterations (None: features.LLOYD_MAX_ITER)
CASES = {"s5000_k100": (100, 3, False, None),
         "s257_k16": (16, 4, False, None),
         "s262444_k8": (8, 5, False, 5),
         "s131201_k5": (5, 8, False, 5),
         "d2_1000_k20": (20, 6, False, None),
         "far_3000_k32": (32, 7, False, None),
         "s1000_k129": (129, 9, False, None),
         "one": (1, 0, True, None),
         "dup64": (64, 2, True, None),
         "lattice": (8, 2, True, None)}
NAMES = list(CASES)


def case_cloud(name):
    from probreg_amd import synthetic

    if name == "one":
        return np.array([[0.3, -0.7, 1.1]])
    if name == "dup64":
        p = synthetic.surface(32, 38)
        return np.concatenate([p, p], axis=0)
    if name == "lattice":
        g = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), np.arange(4.0), indexing="ij"), axis=-1).reshape(-1, 3)
        return g[np.random.default_rng(0).permutation(64)]
    x = {"s5000_k100": (5000, 31), "s257_k16": (257, 32), "s262444_k8": (262444, 33), "s131201_k5": (131201, 36),
         "d2_1000_k20": (1000, 34), "far_3000_k32": (3000, 35), "s1000_k129": (1000, 37)}[name]
    x = synthetic.surface(*x)
    if name == "d2_1000_k20":
        x = np.ascontiguousarray(x[:, :2])
    if name == "far_3000_k32":
        x = x + np.array([1000.0, -2000.0, 500.0])
    return x


@functools.lru_cache(maxsize=None)
def make_case(name):
    from probreg_amd import features

    k, rs, exact, max_iter = CASES[name]
    x = case_cloud(name)
    x.setflags(write=False)
    return {"x": x, "n": x.shape[0], "k": k, "u": features.seed_uniforms(k, rs), "exact": exact,
            "max_iter": features.LLOYD_MAX_ITER if max_iter is None else max_iter,
            "tol": features.lloyd_tolerance(x), "xmax": float(np.max(np.abs(x)))}


@functools.lru_cache(maxsize=None)
def oracle_seed(name):
    c = make_case(name)
    return og.seed(c["x"], c["k"], c["u"], exact=c["exact"])


@functools.lru_cache(maxsize=None)
def oracle_lloyd(name, max_iter=None):
    c = make_case(name)
    idx, _ = oracle_seed(name)
    return og.lloyd(c["x"], c["x"][idx], c["max_iter"] if max_iter is None else max_iter, c["tol"], exact=c["exact"])


@functools.lru_cache(maxsize=None)
def oracle_init(name):
    c = make_case(name)
    return og.init_from_labels(c["x"], oracle_lloyd(name)[3]["labels"], c["k"], REG_COVAR)


def seeding_is_clear(name):
    c = make_case(name)
    _, m = oracle_seed(name)
    bound = og.decision_bound(c["n"])
    winner = float(np.min(m["winner"])) if c["k"] > 1 else np.inf
    sampling = float(np.min(m["sampling"])) if c["k"] > 1 else np.inf
    print("%s: winner margin %.3e sampling margin %.3e bound %.3e" % (name, winner, sampling, bound))
    assert winner >= bound and sampling >= bound


def lloyd_is_clear(name, max_iter=None):
    c = make_case(name)
    _, n_iter, _, m = oracle_lloyd(name, max_iter)
    bound = og.decision_bound(c["n"])
    stop_bound = bound * max(1.0, c["xmax"] / np.sqrt(c["tol"])) if c["tol"] > 0 else bound
    print("%s: %d Lloyd iterations, label gap %.3e, over max(1, max|x| / d) %.3e bound %.3e, stop margin %.3e bound %.3e"
          % (name, n_iter, m["label_gap"], m["label_clear"], bound, m["stop"], stop_bound))
    assert m["label_clear"] >= bound and m["stop"] >= stop_bound


def within(got, ref, scale, n, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    err = float(np.max(np.abs(got - ref)))
    bound = og.decision_bound(n) * float(scale)
    print("%s: err %.3e bound %.3e" % (what, err, bound))
    assert err <= bound, "%s: %.3e, bound %.3e" % (what, err, bound)


def same_params(got, ref, c, what):
    within(got[0], ref[0], np.max(np.abs(ref[0])), c["n"], what + " weights")
    within(got[1], ref[1], c["xmax"], c["n"], what + " means")
    within(got[2], ref[2], c["xmax"] ** 2, c["n"], what + " covariances")


class Fit(object):
    """A plan on the case's cloud, seeded with the case's uniforms."""

    def __init__(self, name):
        from probreg_amd import features

        self.case = make_case(name)
        self.plan = features.GmmFitPlan()

    def __enter__(self):
        self.plan.set_data(self.case["x"])
        self.plan.seed(self.case["k"], self.case["u"])
        return self.plan

    def __exit__(self, *exc):
        self.plan.close()


@pytest.mark.parametrize("name", NAMES)
def test_seeds_equal_the_oracle(name):
    seeding_is_clear(name)
    c = make_case(name)
    idx, _ = oracle_seed(name)
    with Fit(name) as plan:
        got = plan.seeds()
        centers = plan.centers()
    assert got.tolist() == idx.tolist()
    assert np.array_equal(centers, c["x"][idx])


@pytest.mark.parametrize("name,max_iter", [(n, None) for n in NAMES] + [("lattice", 1)])
def test_lloyd_equals_the_oracle(name, max_iter):
    """Iteration count, centres and the label counts of the final centres.  ``lattice`` also stops after one iteration:
    its first assignment has exact ties (asserted), and the centres after the single update show how they were broken."""
    seeding_is_clear(name)
    lloyd_is_clear(name, max_iter)
    c = make_case(name)
    ref_centers, ref_iter, ref_counts, _ = oracle_lloyd(name, max_iter)
    if name == "lattice":
        idx, _ = oracle_seed(name)
        assert og.lloyd(c["x"], c["x"][idx], 1, c["tol"], exact=False)[3]["label_gap"] == 0.0
    if name == "dup64":
        assert int(np.count_nonzero(ref_counts == 0)) == 32
    with Fit(name) as plan:
        n_iter = plan.lloyd(c["max_iter"] if max_iter is None else max_iter, c["tol"])
        centers = plan.centers()
        plan.init_from_labels(REG_COVAR)
        counts = plan.params()[0] * c["n"]
    assert n_iter == ref_iter
    within(centers, ref_centers, c["xmax"], c["n"], "%s centres after %d iterations" % (name, n_iter))
    assert np.max(np.abs(counts - np.rint(counts))) < 1.0e-6
    assert np.rint(counts).astype(np.int64).tolist() == ref_counts.tolist()


@pytest.mark.parametrize("name", NAMES)
def test_init_from_labels_equals_the_oracle(name):
    seeding_is_clear(name)
    lloyd_is_clear(name)
    c = make_case(name)
    ref = oracle_init(name)
    with Fit(name) as plan:
        plan.lloyd(c["max_iter"], c["tol"])
        plan.init_from_labels(REG_COVAR)
        got = plan.params()
    same_params(got, ref, c, name + " start")
    if name == "dup64":
        empty = oracle_lloyd(name)[2] == 0
        assert int(np.count_nonzero(empty)) == 32
        assert np.all(got[1][empty] == 0.0) and np.all(np.abs(got[2][empty] - REG_COVAR) < 1e-20)
        assert np.all(got[0][empty] == og.TEN_EPS / c["n"])


@pytest.mark.parametrize("name", NAMES)
def test_em_iterations_equal_the_oracle(name):
    """One EM iteration from the M-step on the labels, then one from the oracle's result of the first."""
    c = make_case(name)
    x, n = c["x"], c["n"]
    with Fit(name) as plan:
        plan.lloyd(c["max_iter"], c["tol"])
        plan.init_from_labels(REG_COVAR)
        start = plan.params()
        n_iter, conv, lbs = plan.em(1.0e-3, 1, REG_COVAR)
        assert n_iter == 1 and not conv
        first = plan.params()
        ref1 = og.em_step(x, start[0], start[1], start[2], REG_COVAR)
        within(lbs[0], ref1[3], abs(ref1[3]), n, name + " lower bound, iteration 1")
        same_params(first, ref1[:3], c, name + " iteration 1")
        prec = 1.0 / ref1[2]
        plan.set_params(ref1[0], ref1[1], prec)
        n_iter, conv, lbs = plan.em(1.0e-3, 1, REG_COVAR)
        assert n_iter == 1 and not conv
        second = plan.params()
    ref2 = og.em_step(x, ref1[0], ref1[1], None, REG_COVAR, precisions=prec)
    within(lbs[0], ref2[3], abs(ref2[3]), n, name + " lower bound, iteration 2")
    same_params(second, ref2[:3], c, name + " iteration 2")
