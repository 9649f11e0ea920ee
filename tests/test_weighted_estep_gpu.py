"""The weighted (BCPD) E-step on every engine that can run it, per point and per moment against the fp64 numpy oracle
(oracle.bcpd_numpy.expectation_step; reference: probreg/bcpd.py:53-72) of exactly the float32 clouds the plan holds.

A per-source weight a_m rides in z4.w as the extra squared distance q_m = -2 sigma2 ln a_m (k_transform_linear); every sweep adds it
to d^2, the row passes take q p1 back out of their residual channel, the outlier constant takes the caller's ratio for M / N.  Weighted
plans stay off the matrix cores, the single sweeps and the column-minimum seed (estep_layout), which leaves the culled grid, the work
queue and the un-culled packed and scalar sweeps - run here on the cases of tests/weighted_cases.py: a cube, a 10 : 1 : 1 box, two blobs
with empty space between them, a target blob the source lacks (2100 x 1900 points and swapped: no multiple of 32 / 128 / 256 / 512),
sizes around the tile edges, source points of weight zero, weights switched off and on again, and the displacement branch of the
transform.  Every E-step goes through bcpd._estep_on_plan: the production mapping of (alpha, Sigma) to (ln a - max, ratio) is part of
what is tested.  tests/test_weighted_cases.py holds the cases' preconditions on the CPU.

Bounds: the project's own (tests/test_estep_families_gpu.py, tests/test_queue_engine_gpu.py): n_p 2e-6 relative, nu_d 2e-5, nu and px
2e-5 of max(1, largest entry), moments 2e-6 n_p; one engine against another 2e-6 of the largest entry."""
import numpy as np
import pytest

import cloud_families as cf
import weighted_cases as wc
from oracle import bcpd_numpy as bo
from test_estep_families_gpu import _Figures, _stops_at_a_hip_error, _write_state

pytestmark = pytest.mark.gpu

# engine: (sparse engine, (r_col, r_row) of set_tuning, (sort, cull) of set_options)
ENGINES = {
    "grid":     (0, (0, 0), (True, True)),      # grid-culled vector sweeps
    "queue":    (2, (0, 0), (True, True)),      # ... over the work queue
    "cull_off": (0, (0, 0), (True, False)),     # un-culled packed sweeps, 2 points per lane, kd-tree order
    "scalar":   (0, (-2, -4), (True, True)),    # un-culled scalar sweeps (2 points per lane in the column pass, 4 in the row pass)
    "unsorted": (0, (0, 0), (False, True)),     # un-culled packed sweeps in the caller's order (no permutation anywhere)
    # the other register counts of launch_*pass_scalar / launch_*pass_packed (run on three cases)
    "scalar_42": (0, (-4, -2), (True, True)),
    "packed_4":  (0, (4, 4), (True, False)),
}
FIVE = ("grid", "queue", "cull_off", "scalar", "unsorted")
THREE = [wc.wcase("clusters", "mid"), wc.wcase("lopsided", "late"), wc.wcase("aniso", "late")]
DEAD = wc.wcase("clusters", "mid", wset="dead")

_PLANS = {}


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for plan in _PLANS.values():
        plan.close()
    _PLANS.clear()


def _plan(c, engine):
    """The plan holding the centred float32 clouds of a case; one per cloud pair and option set."""
    b = c.base
    sort, cull = ENGINES[engine][2]
    key = (b.family, b.m, b.n, b.dim, sort, cull)
    if key not in _PLANS:
        from probreg_amd.engine import CpdPlan

        s = wc.case_setup(c)
        plan = CpdPlan()
        if not (sort and cull):
            plan.set_options(sort_source=sort, sort_target=sort, cull=cull)
        plan.set_source(s["s32"])
        plan.set_target(s["t32"])
        plan.init_sums()
        plan.init_params(None)
        _PLANS[key] = plan
    return _PLANS[key]


def _configure(plan, engine, dense=0, sparse=None, moments_only=2):
    plan.set_tuning(ENGINES[engine][1][0], 0, ENGINES[engine][1][1], 0)
    plan.set_dense_engine(dense)
    plan.set_sparse_engine(ENGINES[engine][0] if sparse is None else sparse)
    plan.set_moments_only(moments_only)
    plan.set_lean_factor(-1.0)
    plan.init_params(None)   # a new registration: no seeds of an earlier case


def _estep(plan, c, times=2):
    """`times` weighted E-steps from the case's state through the production mapping; the last one's (nu_d, nu, px)."""
    from probreg_amd import bcpd

    b = c.base
    st = wc.case_setup(c)["st_c"]
    alpha, sd = wc.case_weights(c)
    for _ in range(times):
        _write_state(plan, st, b.dim)
        out = bcpd._estep_on_plan(plan, b.n, b.dim, st.scale, alpha, sd, st.sigma2, b.w)
    return out


def _assert_vector_two_sweeps(plan):
    col, row = plan.pair_counts()
    assert plan.last_estep_engines() == (0, 0) and plan.last_estep_fused() == 0
    assert col > 0 and row > 0, (col, row)
    return col, row


def _compare(plan, out, es, src, tgt, label):
    """(nu_d, nu, px) and the plan's moment block against an oracle E-step `es` of the clouds (src, tgt)."""
    from oracle import cpd_numpy as co

    nu_d, nu, px = out
    mom = plan.get_moments()
    ref = co.moments_from_estep(src, tgt, co.EstepResult(es.nu_d, es.nu, es.px, es.n_p))
    f = _Figures(label)
    f.add("n_p", abs(mom[0] - es.n_p), 2e-6 * es.n_p)
    f.add("nu_d", np.max(np.abs(nu_d - es.nu_d)), 2e-5)
    f.add("nu", np.max(np.abs(nu - es.nu)), 2e-5 * max(1.0, es.nu.max()))
    f.add("px", np.max(np.abs(px - es.px)), 2e-5 * max(1.0, np.abs(es.px).max()))
    f.add("Sx,Sy,Sxy", np.max(np.abs(mom[1:16] - ref[1:16])), 2e-6 * es.n_p)
    f.add("Sxx", abs(mom[22] - ref[22]), 2e-6 * es.n_p)
    f.check()
    assert all(np.all(np.isfinite(a)) for a in (nu_d, nu, px, mom[:23]))


def _compare_case(plan, out, c, label):
    s = wc.case_setup(c)
    _compare(plan, out, wc.oracle_estep(c), s["s32"].astype(np.float64), s["t32"].astype(np.float64), label)


def _rows(cases, engines):
    return [pytest.param(c, e, id="%s-%s" % (wc.case_id(c), e)) for c in cases for e in engines]


# ----------------------------------------------------------------------------------------------------------------------------
# a. parity with the oracle: every engine x family x state, one 2-D family, one swapped-size run per family
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows(wc.grid_cases() + wc.two_d_cases() + wc.swapped_cases(), FIVE)
                         + _rows(THREE, ("scalar_42", "packed_4")))
@_stops_at_a_hip_error
def test_every_weighted_engine_matches_the_oracle(c, engine):
    """Two E-steps from one state (the second runs over the first one's transformed cloud, queue sizes and column minima), the
    second compared."""
    plan = _plan(c, engine)
    _configure(plan, engine)
    out = _estep(plan, c)
    _assert_vector_two_sweeps(plan)
    _compare_case(plan, out, c, "%s %s" % (wc.case_id(c), engine))


# ----------------------------------------------------------------------------------------------------------------------------
# b. the guards: a caller who forces the matrix cores / the single sweeps on a weighted plan still gets the weighted sweeps
# ----------------------------------------------------------------------------------------------------------------------------
@_stops_at_a_hip_error
def test_forced_engines_stay_off_a_weighted_plan():
    """set_dense_engine(2) + set_moments_only(1): without weights this plan would run the fused matrix-core sweep (whose staging
    writes ra.w = 0) or the residual-form owner sweep, and deliver no p1 / px."""
    c = wc.wcase("clusters", "mid")
    plan = _plan(c, "grid")
    _configure(plan, "grid", dense=2, sparse=1, moments_only=1)
    try:
        out = _estep(plan, c)
        _assert_vector_two_sweeps(plan)
        assert plan.last_estep_lean() == 0
        _compare_case(plan, out, c, "%s forced" % wc.case_id(c))
    finally:
        _configure(plan, "grid")


# ----------------------------------------------------------------------------------------------------------------------------
# c. same pairs, same numbers: the queue, the un-culled sweeps and the caller's order against the culled grid
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", THREE, ids=wc.case_id)
@_stops_at_a_hip_error
def test_engines_agree_with_the_grid(c):
    b = c.base
    pairs, out = {}, {}
    for engine in ("grid", "queue", "cull_off", "unsorted"):
        plan = _plan(c, engine)
        _configure(plan, engine)
        out[engine] = _estep(plan, c)
        pairs[engine] = _assert_vector_two_sweeps(plan)
    full = float(b.m) * b.n
    print("%s: pairs / (M N): %s" % (wc.case_id(c), "  ".join("%s %.3f, %.3f" % (e, p[0] / full, p[1] / full)
                                                                for e, p in sorted(pairs.items()))))
    f = _Figures("%s against the grid" % wc.case_id(c))
    for engine in ("queue", "cull_off", "unsorted"):
        for what, a, g in zip(("nu_d", "nu", "px"), out[engine], out["grid"]):
            f.add("%s %s" % (engine, what), np.max(np.abs(a - g)), 2e-6 * np.max(np.abs(g)))
    f.check()
    for engine in ("cull_off", "unsorted"):   # (pads included; no culling without the kd-tree order)
        assert pairs[engine][0] >= full and pairs[engine][1] >= full, (engine, pairs[engine])
        for culled in ("grid", "queue"):
            assert pairs[culled][0] <= pairs[engine][0] and pairs[culled][1] <= pairs[engine][1], (culled, pairs[culled])


# ----------------------------------------------------------------------------------------------------------------------------
# d. dead columns and dead rows
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ("grid", "queue"))
@_stops_at_a_hip_error
def test_dead_columns_are_exact_zeros(engine):
    """`lopsided` late: the 475 columns of the blob the source lacks are beyond fp64's reach whatever the weights: nu_d is EXACTLY
    zero there (in the oracle by its den == 0 rule, bcpd.py:64) and nowhere else."""
    c = wc.wcase("lopsided", "late")
    dead = np.arange(c.base.n // 4)
    assert dead.size == 475
    plan = _plan(c, engine)
    _configure(plan, engine)
    out = _estep(plan, c)
    _assert_vector_two_sweeps(plan)
    _compare_case(plan, out, c, "dead columns %s" % engine)
    assert np.all(out[0][dead] == 0.0)
    assert np.array_equal(np.flatnonzero(out[0] == 0.0), dead)
    assert abs(plan.get_moments()[0] - (c.base.n - dead.size)) < 2e-6 * c.base.n


@pytest.mark.parametrize("engine", FIVE)
@_stops_at_a_hip_error
def test_source_points_of_weight_zero(engine):
    """Every 7th source point has ln a_m = -2000 (exactly 0 in fp64; q_m ~ 4000 sigma2 in z4.w): it takes no mass, and it changes
    nothing for the others."""
    dead = wc.dead_rows(DEAD.base.m)
    plan = _plan(DEAD, engine)
    _configure(plan, engine)
    out = _estep(plan, DEAD)
    _assert_vector_two_sweeps(plan)
    print("dead rows %s: max nu %.2e max |px| %.2e" % (engine, out[1][dead].max(), np.abs(out[2][dead]).max()))
    assert np.all(np.abs(out[1][dead]) <= 1e-30) and np.all(np.abs(out[2][dead]) <= 1e-30)
    _compare_case(plan, out, DEAD, "dead rows %s" % engine)


# ----------------------------------------------------------------------------------------------------------------------------
# e. weights on, off and on again on one plan
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows([wc.wcase("clusters", "mid"), wc.wcase("aniso", "late")], ("grid", "queue")))
@_stops_at_a_hip_error
def test_weights_off_and_on_again(c, engine):
    """A weighted E-step, then set_source_weights(None) and a plain one: it culls with the column minima the WEIGHTED step left
    (min (d^2 + q) >= min d^2: an upper bound only) and has to give the plain CPD E-step of the fp64 C oracle all the same - and
    the same numbers as a plain E-step that starts without any seed.  Then uniform weights (every q_m = 0, ratio M / N): the weighted
    path has to reproduce the plain one."""
    b = c.base
    s = wc.case_setup(c)
    st = s["st_c"]
    plain = wc.oracle_plain(c)
    es = bo.EstepResult(plain.pt1, plain.p1, plain.n_p, plain.px, None)
    src, tgt = s["s32"].astype(np.float64), s["t32"].astype(np.float64)
    plan = _plan(c, engine)
    _configure(plan, engine)
    _estep(plan, c, times=1)
    plan.set_source_weights(None)
    _write_state(plan, st, b.dim)
    plan.estep(b.w)
    seeded = _assert_vector_two_sweeps(plan)
    stale = plan.get_estep()
    _compare(plan, stale, es, src, tgt, "%s %s weights off" % (wc.case_id(c), engine))
    plan.init_params(None)   # no seed at all
    _write_state(plan, st, b.dim)
    plan.estep(b.w)
    unseeded = _assert_vector_two_sweeps(plan)
    fresh = plan.get_estep()
    print("%s %s: column-pass pairs / (M N) with the stale seed %.3f, unseeded %.3f" % (
        wc.case_id(c), engine, seeded[0] / (float(b.m) * b.n), unseeded[0] / (float(b.m) * b.n)))
    assert seeded[0] <= unseeded[0]
    if b.state == "late":   # the seed is in use: the cull radius (~0.4) is a fraction of the 10 : 1 : 1 box
        assert seeded[0] < unseeded[0]
    _compare(plan, fresh, es, src, tgt, "%s %s plain, unseeded" % (wc.case_id(c), engine))
    u = wc.WCase(c.base, "uniform")
    again = _estep(plan, u, times=1)
    _assert_vector_two_sweeps(plan)
    _compare(plan, again, es, src, tgt, "%s %s uniform weights" % (wc.case_id(c), engine))
    f = _Figures("%s %s against the unseeded plain E-step" % (wc.case_id(c), engine))
    for name, got in (("stale seed", stale), ("uniform", again)):
        for what, a, g in zip(("nu_d", "nu", "px"), got, fresh):
            f.add("%s %s" % (name, what), np.max(np.abs(a - g)), 2e-6 * np.max(np.abs(g)))
    f.check()


# ----------------------------------------------------------------------------------------------------------------------------
# f. tile edges: fewer points than a group, one more / one less than a block and a chunk
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows(wc.tile_cases(), ("grid", "queue", "cull_off")))
@_stops_at_a_hip_error
def test_tile_edges(c, engine):
    b = c.base
    plan = _plan(c, engine)
    _configure(plan, engine)
    out = _estep(plan, c)
    _assert_vector_two_sweeps(plan)
    assert all(np.all(np.isfinite(a)) for a in out)
    _compare_case(plan, out, c, "%s %s" % (wc.case_id(c), engine))
    if b.w == 0.0:   # a pad's z4.w must never contribute: every column of P sums to one
        print("%s %s: sum nu_d - N = %.2e" % (wc.case_id(c), engine, out[0].sum() - b.n))
        assert abs(out[0].sum() - b.n) <= 2e-6 * b.n


# ----------------------------------------------------------------------------------------------------------------------------
# g. the displacement branch of the transform: z = s R (y + v_hat) + t
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,dim", [(777, 650, 3), (300, 260, 2)], ids=["777x650", "300x260-2d"])
@_stops_at_a_hip_error
def test_displacement_enters_the_transform(m, n, dim):
    """A plan as CombinedBCPD drives it: bcpd_build_g, a weighted E-step, bcpd_solve on a random residual (which leaves v_hat in the
    plan), a similarity with a rotation of 21 and -13 degrees, scale 1.07 and a translation, and a second E-step: the transformed
    source is float32(s R (y + v) + t) of the v the solve returned (one float32 ulp of the largest |z| for a contraction that
    differs), and the E-step is the oracle's at that z."""
    from oracle import cpd_numpy as co
    from probreg_amd import _lib, bcpd
    from probreg_amd.cpd import _params_block
    from probreg_amd.engine import CpdPlan

    g = np.random.default_rng(31)
    src = g.random((m, dim))
    rot, scale, t = cf._rotation((21.0, -13.0), dim), 1.07, np.array([0.03, -0.02, 0.05])[:dim]
    tgt = (scale * src @ rot.T + t + 0.004 * g.standard_normal((m, dim)))[g.permutation(m)[:n]]
    s32, t32, cy, cx = cf.centred(src, tgt)
    y, x = s32.astype(np.float64), t32.astype(np.float64)
    t_c = t + scale * rot @ cy - cx
    dense = co.squared_kernel_sum_closed_form(y, x)
    alpha, sd = wc.weights(m, dim, 0.02 * dense / scale ** 2)   # exponents in [0, 12] at the second E-step
    w = 0.1

    def params(lin, tt, sc, sigma2):
        p = np.zeros(_lib.PRG_NPARAMS)
        p[:13] = _params_block(lin, tt, sc, dim)[:13]
        p[13] = sigma2
        return p

    plan = CpdPlan()
    try:
        plan.set_source(s32)
        plan.bcpd_build_g(1.0)
        plan.set_target(t32)
        plan.set_w(np.zeros((m, dim)))
        plan.set_params(params(np.identity(dim), np.zeros(dim), 1.0, dense))
        bcpd._estep_on_plan(plan, n, dim, 1.0, alpha, sd, dense, w)
        assert np.array_equal(plan.get_tsource(), s32)   # v = 0, identity: the source itself
        v, _sigma_diag = plan.bcpd_solve(2.0, 1.0 / dense ** 2, 0.05 * g.standard_normal((m, dim)))
        assert np.all(np.isfinite(v)) and np.max(np.abs(v)) > 1e-3   # the displacement is no rounding matter (y is O(1))
        sigma2 = 0.02 * dense
        plan.set_params(params(rot, t_c, scale, sigma2))
        out = bcpd._estep_on_plan(plan, n, dim, scale, alpha, sd, sigma2, w)
        _assert_vector_two_sweeps(plan)
        z = scale * (y + v) @ rot.T + t_c
        got = plan.get_tsource()
        f = _Figures("displacement %d x %d" % (m, n))
        f.add("z", np.max(np.abs(got.astype(np.float64) - z.astype(np.float32).astype(np.float64))), 2.4e-7 * np.max(np.abs(z)))
        f.check()
        assert np.max(np.abs(got - (scale * y @ rot.T + t_c))) > 1e3 * 2.4e-7 * np.max(np.abs(z))   # (v is what moved it)
        es = bo.expectation_step(z, x, scale, alpha, sd, sigma2, w)
        assert es.n_p >= 0.4 * n
        _compare(plan, out, es, y, x, "displacement %d x %d E-step" % (m, n))
    finally:
        plan.close()
