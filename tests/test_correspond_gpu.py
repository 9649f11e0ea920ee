"""CPD correspondences (csrc/cpd_correspond.hip) against the fp64 restatement of tests/oracle_correspond.py (the dense
P of the reference's E-step, probreg/cpd.py:71-88, and a stable sort on (-score, index)): the plan-free stage `topk_sweep` at its tile
edges, with ties, segments and biases; `CpdPlan.correspondences` on the cloud families of tests/cloud_families.py and a weighted case
of tests/weighted_cases.py; far points, pads, consistency with the E-step's own sums, independence of the caller's and the plan's
order; and the public API after a registration.

Error budget (exact float32 inputs, identity transform - the plan gets the transformed source already rounded to float32, so the
oracle sees exactly the device's numbers): a score may differ from the oracle's by
    tau = 4e-7 kappa d^2 + 3e-5
- about six float32 roundings on the exponent's argument (differences, squares, the sum, kappa, its product, the final sums), and
the project's pt1 bound of 2e-5 on the denominator in log2 units (2e-5 / ln 2).  Every check prints its largest measured figure."""
import numpy as np
import pytest

import cloud_families as cf
import oracle_correspond as oc
import weighted_cases as wc
from test_estep_families_gpu import _Figures, _stops_at_a_hip_error

pytestmark = pytest.mark.gpu

TAU_REL, TAU_ABS = 4e-7, 3e-5
ULP20 = float(np.spacing(np.float32(20.0)))
K = 4

_PLANS, _TERMS, _TOPK = [], {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for plan in _PLANS:
        plan.close()
    del _PLANS[:]
    _TERMS.clear()
    _TOPK.clear()


# ----------------------------------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------------------------------
def _run_plan(z32, x32, sigma2, w, sort=True, log_weights=None, ratio=0.0):
    """A plan holding z32 as its source under the identity transform, after one two-sweep E-step on the default engines."""
    from probreg_amd.engine import CpdPlan

    plan = CpdPlan()
    _PLANS.append(plan)
    if not sort:
        plan.set_options(sort_source=False, sort_target=False, cull=True)
    plan.set_source(z32)
    plan.set_target(x32)
    plan.init_sums()
    plan.init_params(None)
    plan.set_moments_only(2)
    if log_weights is not None:
        plan.set_source_weights(log_weights, ratio)
    p = plan.get_params()
    p[:9] = np.identity(3).ravel()
    p[9:12] = 0.0
    p[12] = 1.0
    p[13] = sigma2
    plan.set_params(p)
    plan.estep(w)
    assert plan.last_estep_fused() == 0
    return plan


def _stage_terms(owned, streamed, kappa, owned_bias=None, streamed_bias=None):
    """The stage's inputs as oracle terms: score = streamed_bias - kappa (d^2 + q), q = -owned_bias / kappa."""
    o = np.asarray(owned, dtype=np.float64)
    s = np.asarray(streamed, dtype=np.float64)
    ob = np.zeros(o.shape[0]) if owned_bias is None else np.asarray(owned_bias, dtype=np.float64)
    sb = np.zeros(s.shape[0]) if streamed_bias is None else np.asarray(streamed_bias, dtype=np.float64)
    return oc.Terms(o, s, oc.LOG2E / (2.0 * kappa), float(kappa), None, -ob / kappa, None, sb, 0.0, None)


def _check(label, t, side, k, got, orc=None, index_check=True, abs_term=TAU_ABS, extra=None, prob_bound=2e-5):
    """The value checks (no exemptions), distinct in-range indices, and the index check where the oracle's gaps allow it."""
    index, l2, prob = got
    owned = (t.z if side == "source" else t.x).shape[0]
    n_s = (t.x if side == "source" else t.z).shape[0]
    if orc is None:
        orc = oc.topk(t, side, k + 1)
    assert index.shape == (owned, k) and index.dtype == np.int32 and l2.shape == (owned, k) and l2.dtype == np.float32
    assert index.min() >= 0 and index.max() < n_s, "an index outside the streamed cloud (a pad?)"
    srt = np.sort(index, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "an index twice in one row"
    own = np.arange(owned)[:, None]
    idx = index.astype(np.int64)
    best_i, best = orc.index[:, :k], orc.score[:, :k]
    s_ret = oc.score_at(t, side, own, idx)
    tau = TAU_REL * oc.kappa_d2_at(t, side, own, idx) + abs_term   # of the returned pair
    if extra is not None:
        tau = tau + extra(own, idx)
    d_rank = np.abs(s_ret - best)                       # the oracle score of the returned index vs the oracle's j-th best
    d_score = np.abs(l2.astype(np.float64) - s_ret)     # the returned score vs the oracle's score of that pair
    f = _Figures(label)
    print("%s: largest |score - oracle| %.3e, largest rank difference %.3e (tau up to %.3e)"
          % (label, d_score.max(), d_rank.max(), tau.max()))
    f.add("rank/tau", np.max(d_rank / tau), 1.0)
    f.add("score/tau", np.max(d_score / tau), 1.0)
    if prob is not None:
        assert prob.dtype == np.float64   # exp2 of the returned score: to the last bits, and to the last subnormal steps below 2^-1022
        assert np.allclose(prob, np.exp2(l2.astype(np.float64)), rtol=1e-14, atol=1e-323)
        f.add("prob", np.max(np.abs(prob - np.exp2(best))), prob_bound)
    if index_check:
        tau_o = TAU_REL * oc.kappa_d2_at(t, side, own, best_i) + abs_term   # of the oracle's pair: the band is the oracle's alone
        if extra is not None:
            tau_o = tau_o + extra(own, best_i)
        gaps = orc.score[:, :-1] - orc.score[:, 1:]
        up = np.concatenate([np.full((owned, 1), np.inf), gaps[:, :k - 1]], axis=1)
        sure = (up > 2.0 * tau_o) & (gaps[:, :k] > 2.0 * tau_o)
        f.add("exempt", 1.0 - sure.mean(), 0.05)
        wrong = int(np.sum(idx[sure] != best_i[sure]))
        assert wrong == 0, "%s: %d indices differ from the oracle's where its gaps exceed 2 tau" % (label, wrong)
    f.check()


def _distinct_integer_points(g, n, dim, lo=-32, hi=32):
    """n distinct points with integer coordinates: every d^2 is exact in float32."""
    cells = g.choice((hi - lo) ** dim, size=n, replace=False)
    pts = np.stack([(cells // (hi - lo) ** a) % (hi - lo) + lo for a in range(dim)], axis=1)
    return pts.astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# 1. the stage with zero biases: an exact k-nearest-neighbour search at the tile edges, whatever the segments
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("k", [1, 3, 4, 8])
@_stops_at_a_hip_error
def test_stage_is_an_exact_knn_at_the_tile_edges(k, dim):
    """Distinct integer coordinates and kappa = 2^-4: d^2 and the score are exact in float32, so indices AND scores equal the fp64
    oracle's.  Owned counts around the workgroup (and 1), streamed counts around the loop's tile (and 1, and several segments)."""
    from probreg_amd.engine import correspond_tile_shape, topk_sweep

    wg, tile = correspond_tile_shape()
    g = np.random.default_rng(100 * dim + k)
    kappa = 0.0625
    ran = 0
    for n_o in (1, wg - 1, wg, wg + 1):
        for n_s in (1, tile - 1, tile, tile + 1, 1003):
            if k > n_s:
                continue
            owned = _distinct_integer_points(g, n_o, dim)
            streamed = _distinct_integer_points(g, n_s, dim)
            ref = oc.topk_of_scores(oc.stage_scores(owned, streamed, kappa), k)
            index, score = topk_sweep(owned, streamed, kappa, k=k)
            assert np.array_equal(index, ref.index), (n_o, n_s)
            assert np.array_equal(score.astype(np.float64), ref.score), (n_o, n_s)
            ran += 1
    assert ran >= 8
    # segments that do not divide the streamed count; automatic; twice: byte-identical
    owned = _distinct_integer_points(g, wg + 1, dim)
    streamed = _distinct_integer_points(g, 1003, dim)
    ref = oc.topk_of_scores(oc.stage_scores(owned, streamed, kappa), k)
    first = topk_sweep(owned, streamed, kappa, k=k, segments=1)
    assert np.array_equal(first[0], ref.index) and np.array_equal(first[1].astype(np.float64), ref.score)
    for seg in (1, 2, 7, 0):
        again = topk_sweep(owned, streamed, kappa, k=k, segments=seg)
        assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes(), seg


# ----------------------------------------------------------------------------------------------------------------------------
# 2. ties
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 4])
@_stops_at_a_hip_error
def test_stage_ties_rank_by_the_smaller_index(k):
    """Every streamed point twice, at positions i and i + n/2 of a shuffled cloud: the copies score the same bit for bit, the
    smaller position comes first - within a segment (the sweep) and across segments (the merge: with 2 segments the two copies
    are never in the same one)."""
    from probreg_amd.engine import topk_sweep

    g = np.random.default_rng(7 + k)
    half = _distinct_integer_points(g, 500, 3)
    streamed = np.concatenate([half, half])
    owned = _distinct_integer_points(g, 300, 3)
    n = streamed.shape[0]
    ref = oc.topk_of_scores(oc.stage_scores(owned, streamed, 0.0625), k)
    for seg in (1, 2, 7):
        index, score = topk_sweep(owned, streamed, 0.0625, k=k, segments=seg)
        assert np.array_equal(index, ref.index) and np.array_equal(score.astype(np.float64), ref.score), seg
        for row in index:
            pos = {int(j): p for p, j in enumerate(row)}
            assert all(j - n // 2 in pos and pos[j - n // 2] < pos[j] for j in pos if j >= n // 2)
        assert np.array_equal(score[:, 0], score[:, 1]) and np.all(index[:, 0] < n // 2)


@pytest.mark.parametrize("k", [2, 4])
@_stops_at_a_hip_error
def test_plan_ties_rank_by_the_callers_index(k):
    """The same under a plan, where the kernels' order is the kd-tree order: every SOURCE point twice (caller positions i and
    i + M/2, q_m = 0), target side.  The two copies of a source point get the same float32 score for a target point; the copy
    never comes before the original, whatever the plan's internal order."""
    c = cf.case("volume", "mid", 0.1, m=1100, n=1300)
    s = cf.case_setup(c)
    z = cf.transformed(s["st_c"], s["s32"].astype(np.float64)).astype(np.float32)
    half = z.shape[0]
    plan = _run_plan(np.concatenate([z, z]), s["t32"], s["st_c"].sigma2, c.w)
    index, l2, _prob = plan.correspondences(k, "target")
    for row, sc in zip(index, l2):
        pos = {int(j): p for p, j in enumerate(row)}
        assert all(j - half in pos and pos[j - half] < pos[j] and sc[pos[j - half]] == sc[pos[j]] for j in pos if j >= half)
    assert np.all(index[:, 0] < half) and np.array_equal(index[:, 1], index[:, 0] + half)


# ----------------------------------------------------------------------------------------------------------------------------
# 3. biases
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 3])
@_stops_at_a_hip_error
def test_stage_with_biases(dim):
    """A streamed bias in [-20, 0] and an owned bias in [-1, 0] on float32 clouds: scores within tau with the denominator's 3e-5
    replaced by the float32 ulp of 20 (the final sums round at that magnitude), ordering as on a plan."""
    from probreg_amd.engine import topk_sweep

    g = np.random.default_rng(41 + dim)
    owned = g.random((300, dim)).astype(np.float32)
    streamed = g.random((1003, dim)).astype(np.float32)
    ob = (-g.random(300)).astype(np.float32)
    sb = (-20.0 * g.random(1003)).astype(np.float32)
    kappa = float(np.float32(37.3))
    t = _stage_terms(owned, streamed, kappa, ob, sb)
    for seg in (0, 7):
        index, score = topk_sweep(owned, streamed, kappa, k=K, owned_bias=ob, streamed_bias=sb, segments=seg)
        _check("biases %d-D segments %d" % (dim, seg), t, "source", K, (index, score, None), abs_term=ULP20)


# ----------------------------------------------------------------------------------------------------------------------------
# 4. / 5. plans against the oracle
# ----------------------------------------------------------------------------------------------------------------------------
PLAN_CASES = ([cf.case(f, s, 0.1) for f in ("volume", "aniso", "clusters") for s in ("mid", "late")]
              + [cf.case("lopsided", "mid", 0.0), cf.swapped_cases()[2], cf.two_d_cases()[2]])
# (the 2-D case is `clusters late`: in 2-D the `mid` state is nearly flat in the ORACLE - 9 % of the source side's and 36 % of the
# target side's ranks lie within 2 tau of a neighbour in fp64, so the index check would have little left to compare; `late` leaves
# 0.2 %.  The swapped case leaves 4.2 % on its target side, the grid cases at most 3.8 % - the cap of 5 % holds for all of them.)
DENSE_CASE = cf.case("volume", "dense", 0.1)


def _case_terms(c):
    """(oracle terms, plan after its E-step) of a case: the state applied in fp64, rounded to float32 once, identity on the plan."""
    if c not in _TERMS:
        s = cf.case_setup(c)
        z32 = cf.transformed(s["st_c"], s["s32"].astype(np.float64)).astype(np.float32)
        t = oc.terms(z32.astype(np.float64), s["t32"].astype(np.float64), s["st_c"].sigma2, c.w)
        _TERMS[c] = (t, _run_plan(z32, s["t32"], s["st_c"].sigma2, c.w))
    return _TERMS[c]


def _case_topk(c, side):
    if (c, side) not in _TOPK:
        _TOPK[(c, side)] = oc.topk(_case_terms(c)[0], side, K + 1)
    return _TOPK[(c, side)]


@pytest.mark.parametrize("side", ["source", "target"])
@pytest.mark.parametrize("c", PLAN_CASES, ids=cf.case_id)
@_stops_at_a_hip_error
def test_plan_matches_the_oracle(c, side):
    t, plan = _case_terms(c)
    _check("%s %s" % (cf.case_id(c), side), t, side, K, plan.correspondences(K, side), _case_topk(c, side))


@pytest.mark.parametrize("side", ["source", "target"])
@_stops_at_a_hip_error
def test_plan_dense_state_values(side):
    """The registration's initial sigma2: the scores are nearly flat (2 % to 62 % of the ranks lie within 2 tau of a neighbour in
    the oracle itself), so the index check is left out by design; the value checks hold without exemption."""
    t, plan = _case_terms(DENSE_CASE)
    _check("%s %s" % (cf.case_id(DENSE_CASE), side), t, side, K, plan.correspondences(K, side), _case_topk(DENSE_CASE, side),
           index_check=False)


# ----------------------------------------------------------------------------------------------------------------------------
# 6. far points and pads
# ----------------------------------------------------------------------------------------------------------------------------
@_stops_at_a_hip_error
def test_far_points_keep_their_matches_and_pads_never_appear():
    """M = 1025, N = 2049: one above a multiple of 1024, so both clouds end in a block of pads.  Five source points sit 50 extents
    away: every probability of theirs underflows (prob == 0), the score stays finite, and the matches are the oracle's - ranking
    is in the log domain.  (The oracle's gaps at those rows exceed 2 tau, asserted, so equality is exact.)"""
    c = cf.case("volume", "dense", 0.1, m=1025, n=2049)
    s = cf.case_setup(c)
    z = cf.transformed(s["st_c"], s["s32"].astype(np.float64))
    far = np.array([3, 256, 511, 1000, 1024])
    extent = float(np.max(z.max(axis=0) - z.min(axis=0)))
    z[far] += 50.0 * extent * np.array([1.0, 0.3, -0.2])
    z32 = z.astype(np.float32)
    t = oc.terms(z32.astype(np.float64), s["t32"].astype(np.float64), s["st_c"].sigma2, c.w)
    plan = _run_plan(z32, s["t32"], s["st_c"].sigma2, c.w)
    for side in ("source", "target"):
        index, l2, prob = plan.correspondences(K, side)
        n_s = c.n if side == "source" else c.m
        assert index.min() >= 0 and index.max() < n_s and np.all(np.isfinite(l2))
        _check("far %s" % side, t, side, K, (index, l2, prob), index_check=False)
    index, l2, prob = plan.correspondences(K, "source")
    orc = oc.topk(t, "source", K + 1)
    tau = TAU_REL * oc.kappa_d2_at(t, "source", far[:, None], orc.index[far, :K]) + TAU_ABS
    gaps = orc.score[far, :-1] - orc.score[far, 1:]
    assert np.all(gaps[:, :K] > 2.0 * tau), "precondition: the far rows' oracle gaps exceed 2 tau"
    assert np.all(prob[far] == 0.0) and np.all(np.isfinite(l2[far])) and np.all(l2[far] < -1100.0)
    assert np.array_equal(index[far], orc.index[far, :K])
    # and they are simply the nearest targets
    assert np.array_equal(index[far, 0], np.argmin(oc._d2(z32[far].astype(np.float64), t.x), axis=1))


# ----------------------------------------------------------------------------------------------------------------------------
# 7. consistency with the E-step
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,side", [(5, 7, "target"), (7, 5, "source")])
@_stops_at_a_hip_error
def test_all_matches_sum_to_the_esteps_mass(m, n, side):
    """k = 5 takes every streamed point: the probabilities of a row sum to pt1_n (target side) / p1_m (source side) of the same
    E-step within the project's 2e-5."""
    from probreg_amd import cpd

    g = np.random.default_rng(m * 10 + n)
    z = g.random((m, 3))
    x = z[g.integers(0, m, n)] + 0.05 * g.standard_normal((n, 3))
    k = min(m, n)
    r = cpd.correspondences(z, x, 0.01, w=0.1, k=k, side=side)
    assert r.index.shape == ((n if side == "target" else m), k) and r.mass.shape == (r.index.shape[0],)
    assert np.array_equal(np.sort(r.index, axis=1), np.tile(np.arange(k), (r.index.shape[0], 1)))
    err = np.max(np.abs(r.prob.sum(axis=1) - r.mass))
    print("%d x %d %s: |sum_k prob - mass| = %.2e" % (m, n, side, err))
    assert err < 2e-5
    c = x.mean(axis=0)
    t = oc.terms((z - c).astype(np.float32).astype(np.float64), (x - c).astype(np.float32).astype(np.float64), 0.01, 0.1)
    pt1, p1 = oc.sums(t)
    assert np.max(np.abs(r.mass - (pt1 if side == "target" else p1))) < 2e-5


# ----------------------------------------------------------------------------------------------------------------------------
# 8. the caller's order and the plan's order
# ----------------------------------------------------------------------------------------------------------------------------
@_stops_at_a_hip_error
def test_order_independence():
    """Both clouds shuffled: indices map back through the shuffle, scores are byte-identical (the kd-tree order depends on the
    points alone - no two points share a coordinate, asserted).  Without the plan's sorting: the same scores up to what the
    order of the E-step's sums moves b_n by, and the same indices wherever the sorted plan's own scores are further apart than that
    (derived at the assertion)."""
    c = cf.case("volume", "mid", 0.1, m=2100, n=1900)
    s = cf.case_setup(c)
    z32 = cf.transformed(s["st_c"], s["s32"].astype(np.float64)).astype(np.float32)
    x32 = s["t32"]
    for cloud in (z32, x32):
        for a in range(3):
            assert np.unique(cloud[:, a]).size == cloud.shape[0], "precondition: no coordinate twice"
    g = np.random.default_rng(12)
    ps, pt = g.permutation(c.m), g.permutation(c.n)
    sigma2 = s["st_c"].sigma2
    t = oc.terms(z32.astype(np.float64), x32.astype(np.float64), sigma2, c.w)
    plain = _run_plan(z32, x32, sigma2, c.w)
    shuffled = _run_plan(z32[ps], x32[pt], sigma2, c.w)
    unsorted = _run_plan(z32, x32, sigma2, c.w, sort=False)
    for side in ("source", "target"):
        orc = oc.topk(t, side, K + 1)
        a = plain.correspondences(K, side)
        b = shuffled.correspondences(K, side)
        po, pstr = (ps, pt) if side == "source" else (pt, ps)
        assert np.array_equal(a[0][po], pstr[b[0]]), side
        assert a[1][po].tobytes() == b[1].tobytes() and a[2][po].tobytes() == b[2].tobytes(), side
        _check("order %s" % side, t, side, K, a, orc)
        # Without the plan's sorting nothing but the order of the E-step's sums changes: b_n is -log2 of a float32-accumulated
        # denominator, which either plan holds within the project's 2e-5 relative (2.9e-5 in log2 units), so a score of the
        # unsorted plan is within B = 5.8e-5 + 2 float32 ulps of the sorted plan's at the same rank; everything else of a score is
        # the same float32 arithmetic on the same numbers.  Two scores of a row further apart than 2 B cannot change places, so
        # there every index must be the SAME - judged by the sorted plan's own scores (k = 5 gives rank 4 its lower neighbour),
        # with no oracle in between.  Exact identity of all rows cannot hold: b_n differs in its last bits.
        a5 = plain.correspondences(K + 1, side)
        u5 = unsorted.correspondences(K + 1, side)
        assert np.array_equal(a5[0][:, :K], a[0]) and a5[1][:, :K].tobytes() == a[1].tobytes()   # k is a cut, nothing more
        _check("unsorted %s" % side, t, side, K, (u5[0][:, :K].copy(), u5[1][:, :K].copy(), u5[2][:, :K].copy()), orc)
        sa, su = a5[1].astype(np.float64), u5[1].astype(np.float64)
        bound = 5.8e-5 + 2.0 * np.spacing(np.abs(a5[1])).astype(np.float64)
        diff = np.abs(su - sa)
        ulps = np.max(diff / np.spacing(np.abs(a5[1])).astype(np.float64))
        gaps = sa[:, :-1] - sa[:, 1:]
        up = np.concatenate([np.full((sa.shape[0], 1), np.inf), gaps[:, :K - 1]], axis=1)
        same = (up > 2.0 * bound[:, :K]) & (gaps[:, :K] > 2.0 * bound[:, :K])
        print("unsorted vs sorted %s: largest score difference %.3e (%.1f float32 ulps), indices compared on %.2f %% of the ranks, "
              "equal on %.3f %% of all" % (side, diff.max(), ulps, 100.0 * same.mean(), 100.0 * np.mean(u5[0][:, :K] == a[0])))
        assert np.all(diff <= bound), side
        assert same.mean() > 0.9, side
        assert np.array_equal(u5[0][:, :K][same], a[0][same]), side


# ----------------------------------------------------------------------------------------------------------------------------
# 9. the weighted (BCPD) E-step
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["source", "target"])
@_stops_at_a_hip_error
def test_weighted_estep(side):
    """`clusters mid` of tests/weighted_cases.py: log-weights spanning ~17 (q_m up to 40 sigma2) and the caller's uniform ratio, as
    bcpd._estep_on_plan hands them over (ln a - max, exp(-max) / N)."""
    c = wc.wcase("clusters", "mid")
    b = c.base
    if c not in _TERMS:
        s = wc.case_setup(c)
        z32 = cf.transformed(s["st_c"], s["s32"].astype(np.float64)).astype(np.float32)
        lw = wc.log_weights(c)
        top = float(lw.max())
        ratio = float(np.exp(-top) / b.n)
        t = oc.terms(z32.astype(np.float64), s["t32"].astype(np.float64), s["st_c"].sigma2, b.w, lw - top, ratio)
        _TERMS[c] = (t, _run_plan(z32, s["t32"], s["st_c"].sigma2, b.w, log_weights=lw - top, ratio=ratio))
    t, plan = _TERMS[c]
    assert t.q.max() > 20.0 * t.sigma2
    _check("weighted %s %s" % (wc.case_id(c), side), t, side, K, plan.correspondences(K, side))


# ----------------------------------------------------------------------------------------------------------------------------
# 9b. what the plan call refuses
# ----------------------------------------------------------------------------------------------------------------------------
@_stops_at_a_hip_error
def test_plan_call_refuses_a_plan_that_is_not_at_an_estep():
    """prg_cpd_correspond reads b_n, z and sigma2 of ONE E-step: before any E-step, and after everything that writes PARAMS, the
    weights or an E-step result of the caller's, it returns a state error (ProbregHipError, status -3), and an E-step makes it
    valid again.  A plan whose target is a shard of a larger one is refused, and a bad k or side is a ValueError."""
    from probreg_amd import _lib
    from probreg_amd.engine import CpdPlan

    g = np.random.default_rng(5)
    z32 = g.random((300, 3)).astype(np.float32)
    x32 = g.random((280, 3)).astype(np.float32)

    def refused(plan):
        with pytest.raises(_lib.ProbregHipError, match="status -3"):
            plan.correspondences(1, "source")

    def fresh_params(plan):
        p = plan.get_params()
        p[13] = 0.01
        return p

    plan = CpdPlan()
    _PLANS.append(plan)
    plan.set_source(z32)
    plan.set_target(x32)
    plan.init_sums()
    plan.init_params(None)
    plan.set_moments_only(2)
    refused(plan)                                   # no E-step yet
    plan.set_params(fresh_params(plan))
    plan.estep(0.1)
    first = plan.correspondences(2, "source")
    assert first[0].shape == (300, 2)
    pt1, p1, px = plan.get_estep()
    moves = {
        "mstep": lambda: plan.mstep(_lib.PRG_TF_RIGID, True),
        "iterate": lambda: plan.iterate(_lib.PRG_TF_RIGID, True, 0.1, 1),
        "set_params": lambda: plan.set_params(fresh_params(plan)),
        "init_params": lambda: plan.init_params(None),
        "set_source_weights": lambda: plan.set_source_weights(np.full(300, -0.5), 0.0),
        "moments_from_estep": lambda: plan.moments_from_estep(pt1, p1, px),
        "set_target": lambda: plan.set_target(x32),
        "set_source": lambda: plan.set_source(z32),
    }
    for name, move in moves.items():
        move()
        refused(plan)
        if name == "set_source_weights":
            plan.set_source_weights(None, 0.0)
        plan.set_params(fresh_params(plan))
        plan.estep(0.1)
        assert plan.correspondences(1, "target")[0].shape == (280, 1), name
    again = plan.correspondences(2, "source")
    assert np.array_equal(again[0], first[0])       # the same state again: the same matches
    for k, side in ((0, "source"), (9, "source"), (281, "source"), (301, "target")):
        with pytest.raises(ValueError):
            plan.correspondences(k, side)
    with pytest.raises(ValueError):
        plan.correspondences(1, "both")
    # a shard: 280 of 560 target points
    plan.set_target(x32, n_global=560)
    plan.init_sums()
    plan.set_params(fresh_params(plan))
    plan.estep(0.1)
    refused(plan)


# ----------------------------------------------------------------------------------------------------------------------------
# 10. the public API
# ----------------------------------------------------------------------------------------------------------------------------
def _transform_extra(t, side, max_z):
    """2 kappa |d| 6e-8 max|z|, see test_registrations_then_correspondences."""
    def extra(own, idx):
        d2 = oc.kappa_d2_at(t, side, own, idx) / t.kappa
        return 2.0 * t.kappa * np.sqrt(d2) * 6e-8 * max_z
    return extra


@_stops_at_a_hip_error
def test_module_function_on_float64_clouds_far_from_the_origin():
    """cpd.correspondences centres both clouds on the target's fp64 mean before the float32 upload; the oracle sees those float32
    numbers, so the plain budget applies 1300 units from the origin."""
    from probreg_amd import cpd

    c = cf.case("clusters", "mid", 0.1, m=2100, n=1900, far=cf.FAR)
    s = cf.case_setup(c)
    z, x, sigma2 = cf.transformed(s["st"], s["src"]), s["tgt"], s["st"].sigma2
    ctr = x.mean(axis=0)
    t = oc.terms((z - ctr).astype(np.float32).astype(np.float64), (x - ctr).astype(np.float32).astype(np.float64), sigma2, c.w)
    pt1, p1 = oc.sums(t)
    for side in ("source", "target"):
        r = cpd.correspondences(z, x, sigma2, w=c.w, k=K, side=side)
        assert isinstance(r, cpd.Correspondences)
        _check("module function %s" % side, t, side, K, (r.index, r.log2_prob, r.prob))
        assert np.max(np.abs(r.mass - (p1 if side == "source" else pt1))) < 2e-5 * max(1.0, p1.max())
    for bad in (0, 9, c.n + 1):
        with pytest.raises(ValueError):
            cpd.correspondences(z[:50], x[:5] if bad > 9 else x[:60], sigma2, k=(6 if bad > 9 else bad))
    with pytest.raises(ValueError):
        cpd.correspondences(z[:50], x[:60], sigma2, side="both")


@_stops_at_a_hip_error
def test_registrations_then_correspondences():
    """RigidCPD and NonRigidCPD at M = N = 2000, CombinedBCPD at 1000: `.registration`, then `.correspondences`, against the oracle
    at the registration's final state.

    Here the device transforms the source itself: z = T(y) is evaluated in fp64 from the float32 source the plan holds and rounded
    to float32 once (k_transform_linear), so every coordinate of z is off by at most 2^-24 |z_i| and the point by |dz| <= 6e-8 |z|
    <= 6e-8 max|z|.  The oracle takes the fp64 z.  d^2 = |x - z|^2 moves by 2 d . dz + |dz|^2, i.e. by at most 2 |d| 6e-8 max|z|
    (the square is 1e-14 of it), and the score by kappa times that: tau grows by 2 kappa |d| 6e-8 max|z|."""
    from probreg_amd import bcpd, cpd

    def run(label, reg, src, tgt, z_of, w, terms_kw=None):
        ctr = reg._cx
        x32 = (tgt - ctr).astype(np.float32).astype(np.float64)
        z = z_of()
        sigma2 = terms_kw.pop("sigma2")
        t = oc.terms(z, x32, sigma2, w, **terms_kw)
        extra_of = lambda side: _transform_extra(t, side, float(np.max(np.linalg.norm(z, axis=1))))
        for side in ("source", "target"):
            r = reg.correspondences(k=K, side=side)
            _check("%s %s" % (label, side), t, side, K, (r.index, r.log2_prob, r.prob), extra=extra_of(side))
            assert r.mass.shape == (r.index.shape[0],)
        for bad in (0, 9):
            with pytest.raises(ValueError):
                reg.correspondences(k=bad)

    # rigid
    src, tgt = cf.make_clouds("volume", 2000, 2000)
    reg = cpd.RigidCPD(src)
    with pytest.raises(RuntimeError):
        reg.correspondences()
    res = reg.registration(tgt, w=0.1, maxiter=20, tol=-1.0)
    tr = res.transformation
    y32 = (src - reg._cy).astype(np.float32).astype(np.float64)
    t_c = np.asarray(tr.t) + tr.scale * np.asarray(tr.rot) @ reg._cy - reg._cx
    run("RigidCPD", reg, src, tgt, lambda: tr.scale * y32 @ np.asarray(tr.rot).T + t_c, 0.1, {"sigma2": res.sigma2})
    with pytest.raises(ValueError):
        cpd.RigidCPD(src[:5]).correspondences(side="sideways")

    # affine
    src, tgt = cf.make_clouds("aniso", 2000, 2000, seed=9)
    reg = cpd.AffineCPD(src)
    with pytest.raises(RuntimeError):
        reg.correspondences()
    res = reg.registration(tgt, w=0.1, maxiter=20, tol=-1.0)
    tr = res.transformation
    y32 = (src - reg._cy).astype(np.float32).astype(np.float64)
    t_c = np.asarray(tr.t) + np.asarray(tr.b) @ reg._cy - reg._cx
    run("AffineCPD", reg, src, tgt, lambda: y32 @ np.asarray(tr.b).T + t_c, 0.1, {"sigma2": res.sigma2})
    with pytest.raises(NotImplementedError):
        reg.correspondences(target=tgt)

    # non-rigid
    src, tgt = cf.make_clouds("volume", 2000, 2000, seed=6)
    tgt = tgt + 0.02 * np.sin(3.0 * tgt[:, ::-1])
    reg = cpd.NonRigidCPD(src, beta=0.5, lmd=2.0)
    with pytest.raises(RuntimeError):
        reg.correspondences()
    res = reg.registration(tgt, w=0.1, maxiter=6, tol=-1.0)
    y32 = (src - reg._origin).astype(np.float32).astype(np.float64)
    disp = res.transformation.transform(src) - src
    run("NonRigidCPD", reg, src, tgt, lambda: y32 + disp, 0.1, {"sigma2": res.sigma2})

    # constrained non-rigid: the same plan path with correspondence priors in the M-step (alpha = 1: barely trusted)
    src, tgt = cf.make_clouds("volume", 1000, 1000, seed=7)
    tgt = tgt + 0.02 * np.sin(3.0 * tgt[:, ::-1])
    reg = cpd.ConstrainedNonRigidCPD(src, beta=0.5, lmd=2.0, alpha=1.0, idx_source=np.arange(20), idx_target=np.arange(20))
    with pytest.raises(RuntimeError):
        reg.correspondences()
    res = reg.registration(tgt, w=0.1, maxiter=4, tol=-1.0)
    y32 = (src - reg._origin).astype(np.float32).astype(np.float64)
    disp = res.transformation.transform(src) - src
    run("ConstrainedNonRigidCPD", reg, src, tgt, lambda: y32 + disp, 0.1, {"sigma2": res.sigma2})

    # k beyond the streamed count, through a registration object
    small = cpd.RigidCPD(src[:10])
    small.registration(tgt[:6], w=0.1, maxiter=2, tol=-1.0)
    assert small.correspondences(k=6).index.shape == (10, 6) and small.correspondences(k=8, side="target").index.shape == (6, 8)
    with pytest.raises(ValueError):
        small.correspondences(k=7)

    # Bayesian
    src, tgt = cf.make_clouds("volume", 1000, 1000, seed=8)
    reg = bcpd.CombinedBCPD(src, lmd=2.0)
    with pytest.raises(RuntimeError):
        reg.correspondences()
    tr = reg.registration(tgt, w=0.1, maxiter=4, tol=-1.0)
    last = reg._last[0]
    rigid = tr.rigid_trans
    y32 = (src - reg._cy).astype(np.float32).astype(np.float64)
    t_c = np.asarray(rigid.t) + rigid.scale * np.asarray(rigid.rot) @ reg._cy - reg._cx
    lw = np.log(np.maximum(np.broadcast_to(last.alpha, (1000,)), np.finfo(np.float64).tiny)) \
        - rigid.scale ** 2 * 3 / (2.0 * last.sigma2) * np.asarray(last.sigma_mat)
    top = float(lw.max())
    run("CombinedBCPD", reg, src, tgt, lambda: rigid.scale * (y32 + np.asarray(tr.v)) @ np.asarray(rigid.rot).T + t_c, 0.1,
        {"sigma2": last.sigma2, "log_weights": lw - top, "uniform_ratio": float(np.exp(-top) / 1000)})
