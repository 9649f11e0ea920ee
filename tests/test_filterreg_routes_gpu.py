"""The FilterReg plan's lattice choice and E-step on every route prg_fr_estep can take, against the oracle
(oracle/filterreg_numpy.py over the C lattice), with prg_fr_last_route telling which route ran.

The reference decides by building the blurred lattice and counting (filterreg.py:90-91).  The plan remembers the previous
E-step's answer and builds that lattice first, proves "too large" on a sixteenth of the points while it builds the other one,
sizes its hash table from the previous lattice of the same kind (and retries at full capacity), tells builds apart by a
generation stamp instead of clearing the table, embeds "every 16th" and "the others" in two launches, and leaves the slice
step to the point-to-point M-step.  Whole registrations see all that only through a final pose at 1e-4; here every E-step is
held to the oracle's lattice size, decision and arrays - bit for bit with the splat in the reference's order (mode 2), within
3e-5 of the largest value with the default fixed-point splat (the bar of test_filterreg_gpu.test_estep_vs_oracle).

Route 4 (the thresholded build stopped after its first sixteenth) is not reached, and cannot be short of a side-table
overflow: with M + N >= 4096 that sixteenth is the sample the side stage has just hashed with the same scaling and found no
larger than the threshold, and below 4096 points the thresholded build is not staged.  (The side table holds four slots per
entry the sample can create; an overflow is a probe chain of more than 4096 slots.)

Cases and their preconditions: tests/filterreg_routes.py, tests/test_filterreg_routes_cases.py.
"""
import functools

import numpy as np
import pytest

import filterreg_routes as fr

pytestmark = pytest.mark.gpu

MODES = (2, 1)          # the reference's splat order (the reference's bits), the default fixed-point splat
TOL_ESTEP = 3e-5        # default mode, relative to the largest |value| of the array
TOL_TF = 2e-6           # one M-step: rotation entries, translation over max(1, |t|)   (test_filterreg_claim_gpu)
TOL_SIGMA2 = 1e-5       # relative
TOL_Q = 1e-4            # relative
W = 0.05


class _splat_mode(object):
    """prg_lattice_set_splat_mode for the duration of a ``with`` block (1, fixed-point atomics, is the default)."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from probreg_amd import _lib

        _lib.check(_lib.lib.prg_lattice_set_splat_mode(self.mode))

    def __exit__(self, *exc):
        from probreg_amd import _lib

        _lib.check(_lib.lib.prg_lattice_set_splat_mode(1))


def _plan(src, tgt, sigma2, normals=None):
    from probreg_amd import filterreg

    plan = filterreg._Plan()
    plan.set_source(src)
    plan.set_target(tgt)
    if normals is not None:
        plan.set_normals(normals)
    dim = src.shape[1]
    plan.set_state(np.identity(dim), np.zeros(dim), sigma2)
    return plan


def _check_arrays(got, want, mode, what, names=("m0", "m1", "m2")):
    assert len(got) == len(want) == len(names)
    for name, a, b in zip(names, got, want):
        assert a.dtype == np.float32 and a.shape == b.shape, (what, name)
        err = float(np.max(np.abs(a - b)))
        if mode == 2:
            assert np.array_equal(a, b), (what, name, err)
        else:
            assert err <= TOL_ESTEP * float(np.max(np.abs(b))), (what, name, err)


def _check_mstep(out, ms, what):
    """The 18 doubles of prg_fr_mstep against the oracle's M-step; returns the figures."""
    dim = ms.rot.shape[0]
    rot, t = out[:9].reshape(3, 3)[:dim, :dim], out[9:9 + dim]
    e_rot = float(np.max(np.abs(rot - ms.rot)))
    e_t = float(np.max(np.abs(t - ms.t))) / max(1.0, float(np.max(np.abs(ms.t))))
    e_s2 = abs(out[15] - ms.sigma2) / abs(ms.sigma2)
    e_q = abs(out[13] - ms.q) / abs(ms.q)
    print("%s: M-step rot %.2e t %.2e sigma2 %.2e q %.2e" % (what, e_rot, e_t, e_s2, e_q))
    assert e_rot <= TOL_TF and e_t <= TOL_TF and e_s2 <= TOL_SIGMA2 and e_q <= TOL_Q, (what, e_rot, e_t, e_s2, e_q)
    assert out[16] == 1.0   # there was something to fit
    return e_rot, e_t, e_s2, e_q


# ---- a. the alpha script on one plan -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _script_case(name):
    """Clouds, alphas and the oracle's E-step of both decisions - computed once, shared by both splat modes, never changed."""
    _, m, n, dim = fr.SCRIPT_CASES[fr.SCRIPT_IDS.index(name)]
    src, tgt = fr.clouds(m, n, dim)
    alphas = fr.step_alphas(src, tgt, fr.SIGMA2)
    rot, t = np.identity(dim), np.zeros(dim)
    oracle = {}
    for alpha in alphas:
        _, es, info, ms = fr.oracle_step(src, tgt, rot, t, fr.SIGMA2, alpha=alpha, w=W)
        if info[1] not in oracle:
            for a in es[:3]:
                a.setflags(write=False)
            oracle[info[1]] = (es, info, ms)
        assert oracle[info[1]][1] == info
    return src, tgt, alphas, oracle


def test_last_route_needs_an_estep():
    from probreg_amd import _lib

    src, tgt = fr.clouds(200, 300)
    plan = _plan(src, tgt, fr.SIGMA2)
    with pytest.raises(_lib.ProbregHipError):
        plan.last_route()
    plan.estep()
    assert plan.last_route()[0] in (1, 2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", fr.SCRIPT_IDS)
def test_alpha_script_takes_every_route_and_equals_the_oracle(name, mode):
    src, tgt, alphas, oracle = _script_case(name)
    want_script = fr.expected_script(src.shape[0] + tgt.shape[0])
    seen = []
    with _splat_mode(mode):
        plan = _plan(src, tgt, fr.SIGMA2)
        for step, (alpha, (w_blur, w_route, w_builds, w_sampled)) in enumerate(zip(alphas, want_script), 1):
            es, info, _ = oracle[w_blur]
            size, blur = plan.estep(alpha)
            route = plan.last_route()
            seen.append(route)
            assert (size, blur) == info, (name, step, alpha)
            # one table attempt throughout: the first build of a kind has the whole table, the later ones 65536 slots
            # for a few hundred vertices
            assert route == (w_route, w_builds, 1, w_sampled), (name, step, alpha, route)
            _check_arrays(plan.get_estep(True), es[:3], mode, (name, step))
    print("%s mode %d routes: %s" % (name, mode, seen))


# ---- b. the slice fused into the M-step's terms kernel, and flushed before it ------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,steps,want_route", [("tot4096", (0,), 1), ("tot4096", (0, 1, 2), 3), ("flat", (2,), 2)])
def test_fused_and_flushed_slice_are_the_same_floats(name, steps, want_route, mode):
    """Twin plans, the same E-steps (the last one by route `want_route`; the blurred lattice for route 1).  A: M-step, then
    get_estep - k_fr_terms<true> slices and writes the values; B: get_estep, then M-step - k_slice, then k_fr_terms<false>.
    Both slices are specified as the reference's slice arithmetic, so the values are equal bit for bit in either splat mode;
    the two terms kernels then do the same arithmetic on the same floats, in the same workgroups and summation order."""
    src, tgt, alphas, oracle = _script_case(name)
    with _splat_mode(mode):
        a, b = _plan(src, tgt, fr.SIGMA2), _plan(src, tgt, fr.SIGMA2)
        for plan in (a, b):
            for k in steps:
                size, blur = plan.estep(alphas[k])
            assert plan.last_route()[0] == want_route
        es, info, ms = oracle[blur]
        assert (size, blur) == info
        out_a = a.mstep(W, True, "pt2pt", -1.0)
        got_a = a.get_estep(True)
        got_b = b.get_estep(True)
        out_b = b.mstep(W, True, "pt2pt", -1.0)
    what = (name, want_route, mode)
    for x, y in zip(got_a, got_b):
        assert np.array_equal(x, y), what
    _check_arrays(got_a, es[:3], mode, what)
    for tag, out in (("fused", out_a), ("flushed", out_b)):
        _check_mstep(out, ms, "%s route %d mode %d %s" % (name, want_route, mode, tag))
        assert out[17] == fr.SIGMA2 and out[12] == fr.SIGMA2        # min_sigma2 < 0: the device sigma2 stays
    print("fused - flushed M-step outputs: max |diff| %.3e" % float(np.max(np.abs(out_a - out_b))))
    assert np.array_equal(out_a, out_b), what


# ---- c. point-to-plane plan: eight channels, the slice is not deferred ---------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_pt2pl_plan_on_the_rejected_and_the_side_proof_route(mode):
    from probreg_amd import synthetic

    src, tgt, nrm, _ = synthetic.pt2pl_pair(2596, m=1500, seed=9)
    alphas = fr.step_alphas(src, tgt, fr.SIGMA2)
    _, es, info, _ = fr.oracle_step(src, tgt, np.identity(3), np.zeros(3), fr.SIGMA2, alpha=alphas[2], objective_type="pt2pl",
                                    target_normals=nrm)
    assert info[1] is False
    with _splat_mode(mode):
        plan = _plan(src, tgt, fr.SIGMA2, normals=nrm)
        for step, want_route in ((2, (2, 2, 1, 0)), (3, (3, 1, 1, 1))):
            assert plan.estep(alphas[step - 1]) == info, step
            assert plan.last_route() == want_route, step
            m0, m1, _ = plan.get_estep(False)
            _check_arrays((plan.get_nx(), m0, m1), (es.nx, es.m0, es.m1), mode, ("pt2pl", step), names=("nx", "m0", "m1"))


# ---- d. trajectories on one plan ----------------------------------------------------------------------------------------
def _expected_route(last_blur, blur):
    """Route of an E-step with the default alpha from the previous and the present decision; None where either of two is
    legitimate (a blurred lattice after a non-blurred one: 5, and "not blurred" again without the side proof: 6)."""
    if last_blur:
        return 1 if blur else 2
    return 5 if blur else None


@pytest.mark.parametrize("m,n,must_see", [(3000, 3500, {2, 3}), (6000, 9000, {1, 2, 3})])
def test_trajectory_every_step_from_the_plans_own_state(m, n, must_see):
    """Ten EM iterations on one plan; before each the oracle takes the plan's state and does the same iteration.
    At M = 3000, N = 3500 the blurred lattice has 110 vertices at the first sigma2 against N * 0.015 = 52.5 and only grows, for
    every seed and w (tests/test_filterreg_routes_cases.py): that trajectory is route 2, then side proofs.  The larger pair
    starts below its threshold, so its routes are 1, then 2, then 3."""
    from oracle import filterreg_numpy as fo

    src, tgt = fr.clouds(m, n)
    sigma2 = max(float(fo.squared_kernel_sum_f32(src, tgt)), 1.0e-4)
    plan = _plan(src, tgt, sigma2)
    routes, last_blur = [], True
    for it in range(10):
        st = plan.get_state()
        rot, t, s2 = st[:9].reshape(3, 3), st[9:12], st[12]
        _, es, info, ms = fr.oracle_step(src, tgt, rot, t, s2, w=W)
        got_info = plan.estep()
        route = plan.last_route()
        routes.append(route)
        assert got_info == info, (it, s2, route)
        want_route = _expected_route(last_blur, info[1])
        assert route[0] == want_route or (want_route is None and route[0] in (3, 6)), (it, route)
        last_blur = info[1]
        _check_arrays(plan.get_estep(True), es[:3], 1, (m, n, it))
        out = plan.mstep(W, True, "pt2pt", 1.0e-4)
        _check_mstep(out, ms, "trajectory %d x %d iteration %d" % (m, n, it))
        assert out[17] == s2 and out[12] == max(out[15], 1.0e-4)
    print("trajectory %d x %d routes: %s" % (m, n, routes))
    assert must_see <= {r[0] for r in routes}, routes


# ---- e. table sizing: grow past half of the smallest table, shrink again ------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table_case():
    src, tgt = fr.clouds(fr.TABLE_M, fr.TABLE_N)
    oracle, sizes = {}, {}
    for sigma2, alpha in fr.TABLE_STEPS:
        if (sigma2, alpha) not in oracle:
            _, es, info, _ = fr.oracle_step(src, tgt, np.identity(3), np.zeros(3), sigma2, alpha=alpha)
            for a in es[:3]:
                a.setflags(write=False)
            oracle[(sigma2, alpha)] = (es, info)
        if sigma2 not in sizes:
            sizes[sigma2] = fr.lattice_sizes(src, tgt, sigma2)[:2]
    return src, tgt, oracle, fr.table_script(sizes, fr.TABLE_N, fr.TABLE_M + fr.TABLE_N)


@pytest.mark.parametrize("mode", MODES)
def test_table_sized_from_the_previous_lattice_grows_and_shrinks(mode):
    """One plan through tiny and > 32768-vertex lattices of both kinds: the build that outgrows a table sized from a tiny
    predecessor is retried at full capacity (attempts == 2; the blurred one's neighbour look-ups must use that capacity's mask),
    and the small tables that follow sit on slots the large lattices filled, which only their older generation tells apart."""
    src, tgt, oracle, script = _table_case()
    seen = []
    with _splat_mode(mode):
        plan = _plan(src, tgt, fr.TABLE_STEPS[0][0])
        for step, ((sigma2, alpha), (w_blur, w_size, w_route, w_builds, w_att)) in enumerate(zip(fr.TABLE_STEPS, script), 1):
            es, info = oracle[(sigma2, alpha)]
            assert info == (w_size, w_blur)
            plan.set_state(np.identity(3), np.zeros(3), sigma2)
            assert plan.estep(alpha) == info, step
            route = plan.last_route()
            seen.append(route)
            assert route == (w_route, w_builds, w_att, 0), (step, route)
            _check_arrays(plan.get_estep(True), es[:3], mode, ("table", step))
    print("table script mode %d routes: %s" % (mode, seen))
    assert [r[2] for r in seen] == [1, 2, 1, 2, 1, 1, 1, 1]
