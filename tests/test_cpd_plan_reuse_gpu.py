"""One ``engine.CpdPlan`` whose clouds are replaced, against a fresh plan given the same input (csrc/cpd_plan.h: every buffer of
the plan is owning, the clouds' groups are kept or re-created as a whole - csrc/cpd_buffers.h).

Sizes sit around the plan's capacity rule ``cap_for(n) = round_up(n + 17408, 1024)``: a source of 1200 and one of 1500 points share
a capacity (19456: the group is kept), 2300 points need the next one (20480: the group is re-created); the target grows from 1000
to 5000 points and shrinks back.  After every replacement the plan runs ``init_sums``, ``init_params`` and 5 rigid iterations, then
one two-sweep E-step, and the parameter block, the moments, ``p1`` / ``px`` and ``pt1`` are held to the fresh plan's.

Whatever a plan keeps from its previous clouds must not show: the comparison is bit for bit, except over the work queue
(``set_sparse_engine(2)``), where a sweep sizes its units from the previous sweep over that queue, whichever registration ran it -
there the bound is the one tests/test_queue_engine_gpu.py holds the queue to against the grid of culled waves (2e-6: sigma2 and q
each relative to itself, the moments per group of like magnitude, see ``_hold``)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QUEUE_TOL = 2e-6  # tests/test_queue_engine_gpu.py: queue against grid
W_OUTLIER = 0.1


def _cloud(n, seed):
    from probreg_amd import synthetic

    src, tgt, _ = synthetic.rigid_pair(n, m=n, seed=seed)
    return src.astype(np.float32), tgt.astype(np.float32)


def _new_plan(sparse_engine=None):
    from probreg_amd import engine

    plan = engine.CpdPlan()
    if sparse_engine is not None:
        plan.set_sparse_engine(sparse_engine)
    return plan


def _register(plan):
    """init_sums, init_params, 5 rigid iterations (single sweeps), one two-sweep E-step: everything the plan then holds."""
    from probreg_amd import _lib

    plan.init_sums()
    plan.init_params()
    plan.iterate(_lib.PRG_TF_RIGID, True, W_OUTLIER, 5)
    out = {"params": plan.get_params(), "moments_iterate": plan.get_moments(), "pt1_iterate": plan.get_estep_pt1()}
    plan.estep(W_OUTLIER)
    out["moments"] = plan.get_moments()
    out["pt1"], out["p1"], out["px"] = plan.get_estep()
    return out


# MOMENTS in groups of like magnitude (include/probreg_hip.h): S0, Sx, Sy, Sxy, Syy, Sxx, the reserved / zeroed rest
MOMENT_GROUPS = ((0, 1), (1, 4), (4, 7), (7, 16), (16, 22), (22, 23), (23, 32))


def _hold(got, want, tol):
    """tol == 0: bit for bit.  Otherwise the forms tests/test_queue_engine_gpu.py uses between the queue and the grid: sigma2 and q
    each relative to itself, what is of the size of the points (rotation, translation, scale; pt1, p1, px) relative to
    max(1, max |.|).  The moments are sums of like terms per group of MOMENT_GROUPS - a different summation order moves every
    entry of a group by a fraction of the group's largest - so each group is held relative to its own largest entry, with no
    floor: a group that is zero stays zero."""
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if tol == 0.0:
            assert np.array_equal(g, w), name
        elif name == "params":
            figures = {"linear, t, scale": np.max(np.abs(g[:13] - w[:13])) / max(1.0, float(np.max(np.abs(w[:13])))),
                       "sigma2": abs(g[13] - w[13]) / w[13], "q": abs(g[14] - w[14]) / abs(w[14]),
                       "n_p": abs(g[15] - w[15]) / w[15]}
            print(name, figures)
            assert all(v <= tol for v in figures.values()), figures
            assert np.array_equal(g[16:], w[16:]), "iteration counter / reserved"
        elif name.startswith("moments"):
            for lo, hi in MOMENT_GROUPS:
                diff, scale = float(np.max(np.abs(g[lo:hi] - w[lo:hi]))), float(np.max(np.abs(w[lo:hi])))
                print(name, (lo, hi), diff, scale)
                assert diff <= tol * scale, (name, lo, hi, diff, scale)
        else:
            diff, scale = float(np.max(np.abs(g - w))), max(1.0, float(np.max(np.abs(w))))
            print(name, diff, scale)
            assert diff <= tol * scale, (name, diff, scale)


@pytest.mark.parametrize("sparse_engine,tol", [(None, 0.0), (0, 0.0), (2, QUEUE_TOL)])
def test_replaced_clouds_register_like_a_fresh_plan(sparse_engine, tol):
    sources = {m: _cloud(m, 100 + m)[0] for m in (1200, 1500, 2300)}
    targets = {1000: _cloud(1000, 7)[1], 5000: _cloud(5000, 8)[1], -1000: _cloud(1000, 9)[1]}
    # (what is replaced, its key): same source capacity, next source capacity, target grows, target shrinks
    steps = [("source", 1500), ("source", 2300), ("target", 5000), ("target", -1000)]
    plan = _new_plan(sparse_engine)
    try:
        src, tgt = sources[1200], targets[1000]
        plan.set_source(src)
        plan.set_target(tgt)
        _register(plan)
        for which, key in steps:
            if which == "source":
                src = sources[key]
                plan.set_source(src)
            else:
                tgt = targets[key]
                plan.set_target(tgt)
            got = _register(plan)
            fresh = _new_plan(sparse_engine)
            try:
                fresh.set_source(src)
                fresh.set_target(tgt)
                want = _register(fresh)
            finally:
                fresh.close()
            _hold(got, want, tol)
    finally:
        plan.close()


def test_source_weights_go_with_the_source():
    """Weights, then a new source: the E-step is a fresh unweighted plan's."""
    src_a, tgt = _cloud(1200, 21)
    src_b = _cloud(1500, 22)[0]

    def estep(plan):
        plan.init_sums()
        plan.init_params()
        plan.estep(W_OUTLIER)
        pt1, p1, px = plan.get_estep()
        return {"moments": plan.get_moments(), "pt1": pt1, "p1": p1, "px": px}

    plan, fresh = _new_plan(), _new_plan()
    try:
        plan.set_source(src_a)
        plan.set_target(tgt)
        plan.set_source_weights(-np.random.default_rng(3).uniform(0.0, 2.0, 1200))
        weighted = estep(plan)
        plan.set_source(src_b)
        got = estep(plan)
        fresh.set_source(src_b)
        fresh.set_target(tgt)
        want = estep(fresh)
    finally:
        plan.close()
        fresh.close()
    _hold(got, want, 0.0)
    assert not np.array_equal(weighted["pt1"], want["pt1"])  # (the weights did reach the first E-step)


def test_dense_solve_after_a_lowrank_one_on_a_smaller_source():
    """build_g (factor), E-step, M-step at M = 700; a source of 900 points; dense build_g, E-step, M-step: W is a fresh plan's."""
    from probreg_amd import synthetic

    src_a, tgt = synthetic.nonrigid_pair(800, m=700, seed=31)
    src_b = synthetic.nonrigid_pair(800, m=900, seed=32)[0]
    beta, lmd = 2.0, 2.0

    def em(plan):
        plan.build_g(beta)
        plan.init_sums()
        plan.init_params()
        plan.estep(0.0)
        plan.mstep_nonrigid(lmd)
        plan.get_params()  # (reports a pivot failure of the M-step)
        return plan.get_w()

    plan, fresh = _new_plan(), _new_plan()
    try:
        plan.set_source(src_a)
        plan.set_target(tgt)
        em(plan)
        assert plan.nonrigid_rank() > 0
        plan.set_source(src_b)
        plan.set_nonrigid_solver(0)
        got = em(plan)
        assert plan.nonrigid_rank() == 0
        fresh.set_nonrigid_solver(0)
        fresh.set_source(src_b)
        fresh.set_target(tgt)
        want = em(fresh)
    finally:
        plan.close()
        fresh.close()
    assert np.array_equal(got, want)


def test_two_dense_bcpd_solves_after_a_grown_source():
    rng = np.random.default_rng(41)
    src_a, src_b = rng.uniform(-12.0, 12.0, (450, 3)), rng.uniform(-12.0, 12.0, (600, 3))
    nu = rng.uniform(0.0, 2.0, 600)
    resid = [rng.normal(0.0, 0.3, (600, 3)) for _ in range(2)]
    lmd, cfac = 2.0, 37.5

    plan, fresh = _new_plan(), _new_plan()
    try:
        plan.set_source(src_a)
        plan.bcpd_build_g(1.0)
        plan.bcpd_solve(lmd, cfac, resid[0][:450], nu[:450])
        plan.set_source(src_b)
        plan.bcpd_build_g(1.0)
        got = [plan.bcpd_solve(lmd, cfac, r, nu) for r in resid]
        fresh.set_source(src_b)
        fresh.bcpd_build_g(1.0)
        want = [fresh.bcpd_solve(lmd, cfac, r, nu) for r in resid]
    finally:
        plan.close()
        fresh.close()
    for (v, sd), (v0, sd0) in zip(got, want):
        assert np.array_equal(v, v0) and np.array_equal(sd, sd0)
    assert not np.array_equal(got[0][0], got[1][0])


def test_correspondence_workspace_grows_once_and_is_reused():
    """k = 1, 8, 2 on one plan: the workspace grows for k = 8 and serves k = 2 as it is; each result is a fresh plan's."""
    src, tgt = _cloud(1200, 51)

    def after_estep(plan):
        plan.set_source(src)
        plan.set_target(tgt)
        plan.init_sums()
        plan.init_params()
        plan.estep(W_OUTLIER)

    plan = _new_plan()
    try:
        after_estep(plan)
        for k in (1, 8, 2):
            got = plan.correspondences(k)
            fresh = _new_plan()
            try:
                after_estep(fresh)
                want = fresh.correspondences(k)
            finally:
                fresh.close()
            for a, b in zip(got, want):
                assert np.array_equal(a, b), k
    finally:
        plan.close()
