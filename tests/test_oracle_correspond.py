"""The fp64 restatement behind the correspondence tests (tests/oracle_correspond.py) against the project's E-step oracle
(oracle/cpd_numpy.py; reference: probreg/cpd.py:71-88), host only: its dense P sums to that oracle's pt1 and p1, it honours the
zero-denominator rule of cpd.py:81 where columns underflow in fp64, and its stable sort ranks equal scores by the smaller index."""
import numpy as np

import cloud_families as cf
import oracle_correspond as oc
from oracle import cpd_numpy as co


def _plan_clouds(c):
    s = cf.case_setup(c)
    return cf.transformed(s["st_c"], s["s32"].astype(np.float64)), s["t32"].astype(np.float64), s["st_c"].sigma2


def test_dense_p_sums_to_the_estep_oracle():
    for c in (cf.case("volume", "mid", 0.1, m=1100, n=1300), cf.case("clusters", "late", 0.0, m=1300, n=1100)):
        z, x, sigma2 = _plan_clouds(c)
        t = oc.terms(z, x, sigma2, c.w)
        pt1, p1 = oc.sums(t)
        es = co.expectation_step(z, x, sigma2, c.w)
        err = max(np.max(np.abs(pt1 - es.pt1)), np.max(np.abs(p1 - es.p1)))
        print("%s: max |pt1, p1 - E-step oracle| = %.2e" % (cf.case_id(c), err))
        assert err < 1e-12
        # s is log2 of that P wherever P is representable
        lo, hi = 100, 164
        p = oc.posterior_rows(t, lo, hi)
        s = oc.score_block(t, "source", lo, hi)
        ok = p > 1e-300
        assert ok.any() and np.max(np.abs(np.log2(p[ok]) - s[ok])) < 1e-9 * max(1.0, np.max(np.abs(s[ok])))
        # the two sides and the pairwise form are one function
        st = oc.score_block(t, "target", 7, 9)
        assert np.max(np.abs(st - oc.score_block(t, "source", 0, c.m)[:, 7:9].T)) < 1e-9
        pairs = np.stack([oc.score_at(t, "target", np.full(c.m, n), np.arange(c.m)) for n in (7, 8)])
        assert np.max(np.abs(st - pairs)) < 1e-9


def test_zero_denominator_rule_on_underflowed_columns():
    """`lopsided` late: the 2250 columns of the blob the source lacks underflow in fp64.  den = float32 eps there (cpd.py:81), the
    column of P is zero, and the score stays finite and ranked."""
    c = cf.case("lopsided", "late", 0.0)
    z, x, sigma2 = _plan_clouds(c)
    t = oc.terms(z, x, sigma2, c.w)
    dead = cf.dead_columns(c.family, c.n)
    assert dead.size == 2250 and np.array_equal(np.flatnonzero(t.zero), dead)
    assert np.all(t.den[dead] == oc.EPS32) and np.allclose(t.b[dead], 23.0, rtol=0, atol=1e-12)
    assert np.all(cf.oracle_estep(c).pt1[dead] == 0.0)   # (the project's E-step oracle zeroes the same columns)
    p = oc.posterior_rows(t, 0, 256)
    assert np.all(p[:, dead] == 0.0)
    # the first 256 target points are dead columns: finite scores, ranked by distance - the best source is the nearest one
    r = oc.topk_of_scores(oc.score_block(t, "target", 0, 256), 3)
    assert np.all(np.isfinite(r.score)) and np.all(r.score < -1000.0)
    assert np.array_equal(r.index[:, 0], np.argmin(oc._d2(x[:256], z), axis=1))


def test_equal_scores_rank_by_the_smaller_index():
    g = np.random.default_rng(3)
    half = g.integers(-20, 20, size=(300, 3)).astype(np.float64)
    half = np.unique(half, axis=0)
    n = half.shape[0]
    streamed = np.concatenate([half, half])
    owned = g.integers(-20, 20, size=(40, 3)).astype(np.float64)
    s = oc.stage_scores(owned, streamed, 0.25)
    r = oc.topk_of_scores(s, 4)
    # the definition, spelled out: order by (-score, index)
    for row in range(owned.shape[0]):
        assert np.array_equal(r.index[row], np.lexsort((np.arange(2 * n), -s[row]))[:4])
    # a point and its copy score the same, and the copy (the larger index) never comes first
    assert np.array_equal(r.score[:, 0], r.score[:, 1])
    for row in range(owned.shape[0]):
        pos = {int(j): p for p, j in enumerate(r.index[row])}
        assert all(j - n in pos and pos[j - n] < pos[j] for j in pos if j >= n)
    assert np.all(r.index[:, 0] < n)
    # both paths of topk_of_scores agree with the plain stable sort
    full = np.argsort(-s, axis=1, kind="stable")[:, :5]
    assert np.array_equal(oc.topk_of_scores(s, 5).index, full)
    assert np.array_equal(oc.topk_of_scores(s[:, :20], 5).index, np.argsort(-s[:, :20], axis=1, kind="stable")[:, :5])
