"""Every rigid / affine CPD E-step engine on clouds that are no surface (tests/cloud_families.py: a cube, a 10 : 1 : 1 box, two
blobs with empty space between them, a target blob the source lacks), per point and per moment against the fp64 C oracle
(reference: probreg/cpd.py:71-88) of exactly the float32 clouds the plan holds.

Which pairs an engine evaluates depends on geometry - group and chunk boxes, the kd-tree order, the column-minimum seed of the cull
bound plus the motion bound, the engine switch's pair counts - and on a surface every block has close neighbours: a wrong box on a
partly padded group, a bound that drops a needed block between two clusters, a column block culled whole, a stale seed after a jump
of the state would go unseen there.  Both sizes (8200 / 9001 and swapped) are above the matrix-core threshold and no multiple of
32 / 128 / 256 / 1024.  Each case runs the E-step twice from one state (the second culls with the first one's seeds) and compares
the second.  tests/test_cloud_families.py holds the cases' preconditions (mass left, no column near fp64's underflow, amplification).

Bounds: the project's own (tests/test_mfma_gpu.py, tests/test_resid_gpu.py): n_p 2e-6 relative, pt1 2e-5, p1 and px 2e-5 of
max(1, largest entry), moments 2e-6 n_p."""
import functools

import numpy as np
import pytest

import cloud_families as cf

pytestmark = pytest.mark.gpu

# engine: (dense engine, sparse engine, moments_only, lean factor or None for the default)
ENGINES = {
    "grid":        (0, 0, 2, None),   # grid-culled vector sweeps, column pass + row pass
    "queue":       (0, 2, 2, None),   # ... over the work queue
    "resid_grid":  (0, 0, 1, None),   # residual-form single sweep on the grid
    "resid_queue": (0, 2, 1, None),   # ... on the queue
    "owner":       (0, 1, 1, None),   # the plan's own single sweep on the vector pipe: the owner sweep
    "mfma_lean":   (2, 1, 2, None),   # matrix-core column pass + lean row pass
    "mfma_full":   (2, 1, 2, 0.0),    # ... + full row pass
    "fused":       (2, 1, 1, None),   # fused matrix-core sweep
    "own":         (1, 1, 1, None),   # whatever the plan chooses for a rigid iteration
}
VECTOR = ("grid", "queue", "resid_grid", "resid_queue", "owner")
MATRIX = ("mfma_lean", "mfma_full", "fused")
# what the ABI reports after an E-step of each engine: (column engine, row engine), single sweep, lean row pass
REPORTS = {"grid": ((0, 0), 0, 0), "queue": ((0, 0), 0, 0), "resid_grid": ((0, 0), 1, 0), "resid_queue": ((0, 0), 1, 0),
           "owner": ((0, 0), 1, 0), "mfma_lean": ((1, 1), 0, 1), "mfma_full": ((1, 1), 0, 0), "fused": ((1, 0), 1, 0)}

_PLANS = {}


def _stops_at_a_hip_error(fn):
    """A HIP error ends the session: nothing more is started on a device that has reported one."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        from probreg_amd import _lib

        try:
            return fn(*args, **kwargs)
        except _lib.ProbregHipError as exc:
            if "status -2" in str(exc):   # PRG_ERR_HIP
                pytest.exit("HIP error in %s: %s" % (fn.__name__, exc), returncode=3)
            raise
    return wrapper


@pytest.fixture(scope="module", autouse=True)
def _close_plans():
    yield
    for plan, _init in _PLANS.values():
        plan.close()
    _PLANS.clear()


def _plan(c, sort=True, cull=True):
    """(plan, init block) holding the centred float32 clouds of a case; one per cloud pair and option set."""
    key = (c.family, c.m, c.n, c.dim, c.far, sort, cull)
    if key not in _PLANS:
        s = cf.case_setup(c)
        if c.far is not None:
            # through the registrar: ITS fp64 centring, checked against the oracle on the clouds as generated
            from probreg_amd import cpd

            reg = cpd.RigidCPD(s["src"])
            reg._initialize(s["tgt"])
            assert np.array_equal(reg._cy, s["cy"]) and np.array_equal(reg._cx, s["cx"])
            _PLANS[key] = (reg._plan, reg._init_block)
        else:
            from probreg_amd.engine import CpdPlan

            plan = CpdPlan()
            if not (sort and cull):
                plan.set_options(sort_source=sort, sort_target=sort, cull=cull)
            plan.set_source(s["s32"])
            plan.set_target(s["t32"])
            plan.init_sums()
            plan.init_params(None)
            _PLANS[key] = (plan, None)
    return _PLANS[key]


def _configure(plan, init, engine):
    dense, sparse, moments_only, lean = ENGINES[engine]
    plan.set_dense_engine(dense)
    plan.set_sparse_engine(sparse)
    plan.set_moments_only(moments_only)
    plan.set_lean_factor(-1.0 if lean is None else lean)
    plan.init_params(init)   # a new registration: no seeds of an earlier case, the engine switch starts over


def _write_state(plan, st_c, dim):
    p = plan.get_params()
    lin = np.identity(3)
    lin[:dim, :dim] = st_c.lin
    p[:9] = lin.ravel()
    p[9:12] = 0.0
    p[9:9 + dim] = st_c.t
    p[12] = st_c.scale
    p[13] = st_c.sigma2
    plan.set_params(p)


def _estep(plan, c, times=2):
    st_c = cf.case_setup(c)["st_c"]
    for _ in range(times):
        _write_state(plan, st_c, c.dim)
        plan.estep(c.w)


def _assert_engine(plan, engine):
    col, row = plan.pair_counts()
    got = (plan.last_estep_engines(), plan.last_estep_fused(), plan.last_estep_lean())
    assert got == REPORTS[engine], (engine, got)
    assert col > 0 and (row > 0) == (REPORTS[engine][1] == 0), (engine, col, row)
    return col, row


class _Figures(object):
    """Collects (what, error, bound), prints every figure, then asserts them all."""

    def __init__(self, label):
        self.label, self.rows = label, []

    def add(self, what, err, bound):
        self.rows.append((what, float(err), float(bound)))

    def check(self):
        print("%s: %s" % (self.label, "  ".join("%s %.2e (< %.1e)" % r for r in self.rows)))
        bad = ["%s %.3e >= %.3e" % r for r in self.rows if not r[1] < r[2]]
        assert not bad, "%s: %s" % (self.label, "; ".join(bad))


def _compare_points(plan, c, label, fig=None):
    """pt1, p1, px and n_p of a two-sweep E-step against the oracle's."""
    es = cf.oracle_estep(c)
    mom = plan.get_moments()
    pt1, p1, px = plan.get_estep()
    if c.far is not None:
        px = px + np.outer(p1, cf.case_setup(c)["cx"])   # the plan works on the centred target
    f = fig or _Figures(label)
    f.add("n_p", abs(mom[0] - es.n_p), 2e-6 * es.n_p)
    f.add("pt1", np.max(np.abs(pt1 - es.pt1)), 2e-5)
    f.add("p1", np.max(np.abs(p1 - es.p1)), 2e-5 * max(1.0, es.p1.max()))
    f.add("px", np.max(np.abs(px - es.px)), 2e-5 * max(1.0, np.abs(es.px).max()))
    if fig is None:
        f.check()
    return pt1


def _compare_moments(plan, c, label, fig=None):
    """pt1, n_p and the moments a rigid M-step reads (MOMENTS[0:16], tr Syy in [16], [22]) of a single sweep against the moments of
    the oracle's E-step."""
    from oracle import cpd_numpy as co

    assert c.far is None
    s = cf.case_setup(c)
    es = cf.oracle_estep(c)
    ref = co.moments_from_estep(s["s32"].astype(np.float64), s["t32"].astype(np.float64), es)
    mom = plan.get_moments()
    pt1 = plan.get_estep_pt1()
    f = fig or _Figures(label)
    f.add("n_p", abs(mom[0] - es.n_p), 2e-6 * es.n_p)
    f.add("pt1", np.max(np.abs(pt1 - es.pt1)), 2e-5)
    f.add("Sx,Sy,Sxy", np.max(np.abs(mom[1:16] - ref[1:16])), 2e-6 * es.n_p)
    f.add("trSyy", abs(mom[16] - (ref[16] + ref[19] + ref[21])), 2e-6 * es.n_p)
    f.add("Sxx", abs(mom[22] - ref[22]), 2e-6 * es.n_p)
    assert np.all(mom[17:22] == 0.0)
    if fig is None:
        f.check()
    return pt1


def _compare(plan, c, engine, label):
    single = plan.last_estep_fused() == 1
    assert engine == "own" or single == (REPORTS[engine][1] == 1)
    return (_compare_moments if single else _compare_points)(plan, c, label)


def _rows(cases, engines_of):
    return [pytest.param(c, e, id="%s-%s" % (cf.case_id(c), e)) for c in cases for e in engines_of(c)]


def _engines_of_state(c):
    # beyond amplification 64 / 256 the lean row pass / the fused sweep are left by specification: no late state on the matrix cores
    return VECTOR + (MATRIX if c.state in ("dense", "mid") else ())


# ----------------------------------------------------------------------------------------------------------------------------
# a. per-point and moment parity: every engine x family x state x w, one 2-D family, one swapped-size run per family
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows(cf.grid_cases() + cf.two_d_cases() + cf.swapped_cases(), _engines_of_state))
@_stops_at_a_hip_error
def test_every_engine_matches_the_oracle(c, engine):
    plan, init = _plan(c)
    _configure(plan, init, engine)
    _estep(plan, c)
    _assert_engine(plan, engine)
    _compare(plan, c, engine, "%s %s" % (cf.case_id(c), engine))


# ----------------------------------------------------------------------------------------------------------------------------
# b. column blocks without any source point in reach
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", VECTOR)
@_stops_at_a_hip_error
def test_dead_column_blocks_are_exact_zeros(engine):
    """`lopsided` late: the 2250 columns of the blob the source lacks are further than fp64 can see (their exponents are beyond
    -760): pt1 is EXACTLY zero there - in the oracle by its den == 0 rule (cpd.py:81), on the GPU in whole culled column blocks -
    and every other column and every row stays within the bounds (p1 reaches ~1600: the source's rim takes the nearby mass)."""
    c = cf.case("lopsided", "late", 0.0)
    dead = cf.dead_columns(c.family, c.n)
    assert dead.size == 2250
    plan, init = _plan(c)
    _configure(plan, init, engine)
    _estep(plan, c)
    _assert_engine(plan, engine)
    pt1 = _compare(plan, c, engine, "dead columns %s" % engine)
    assert np.all(pt1[dead] == 0.0)
    assert np.array_equal(np.flatnonzero(pt1 == 0.0), dead)
    assert abs(plan.get_moments()[0] - (c.n - dead.size)) < 2e-6 * c.n


# ----------------------------------------------------------------------------------------------------------------------------
# c. a jump of the state: the seed is stale, the motion bound alone protects the cull
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows(cf.jump_cases(), lambda c: ("grid", "queue", "own")))
@_stops_at_a_hip_error
def test_state_jump_with_a_stale_seed(c, engine):
    """E-step at `mid`; then the pose hops (rotation 5 and 5 degrees further about z and x, scale 1.05: the source moves by up to
    0.55) with sigma2 50 x smaller, and ONE E-step runs: its cull bound is the previous state's column minima widened by how far
    the source moved.  `jump_deep` (800 x smaller) is the case that needs that widening: a tenth of the columns have their
    nearest source point beyond the 2^-48 radius of the new sigma2 alone."""
    before = c._replace(state="mid")
    plan, init = _plan(c)
    _configure(plan, init, engine)
    _estep(plan, before, times=1)
    _estep(plan, c, times=1)
    col, _row = plan.pair_counts()
    assert col > 0
    if engine != "own":
        _assert_engine(plan, engine)
    _compare(plan, c, engine, "%s %s" % (cf.case_id(c), engine))


# ----------------------------------------------------------------------------------------------------------------------------
# d. culling and the storage order change which pairs are evaluated, never the result
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [cf.case("clusters", "mid", 0.0), cf.case("lopsided", "late", 0.0), cf.case("aniso", "late", 0.1)],
                         ids=cf.case_id)
@_stops_at_a_hip_error
def test_culling_and_order_are_exact(c):
    pairs, out = {}, {}
    for name, sort, cull in (("default", True, True), ("cull off", True, False), ("unsorted", False, True)):
        plan, init = _plan(c, sort=sort, cull=cull)
        _configure(plan, init, "grid")
        _estep(plan, c)
        assert plan.last_estep_engines() == (0, 0) and plan.last_estep_fused() == 0
        pairs[name] = plan.pair_counts()
        assert pairs[name][0] > 0 and pairs[name][1] > 0
        out[name] = _compare_points(plan, c, "%s %s" % (cf.case_id(c), name))
    full = float(c.m) * c.n
    ratio = tuple(pairs["default"][k] / pairs["cull off"][k] for k in (0, 1))
    print("%s: culled / unculled pairs: column pass %.3f, row pass %.3f (unculled / (M N): %.3f, %.3f)" % (
        cf.case_id(c), ratio[0], ratio[1], pairs["cull off"][0] / full, pairs["cull off"][1] / full))
    assert pairs["cull off"][0] >= full and pairs["cull off"][1] >= full   # (pads included)
    assert pairs["unsorted"][0] >= full and pairs["unsorted"][1] >= full   # (no culling without the kd-tree order)
    assert ratio[0] <= 1.0 and ratio[1] <= 1.0, ratio
    if c.family == "clusters":
        assert ratio[0] < 0.6 and ratio[1] < 0.6, "culled / unculled pairs %.3f, %.3f: the blobs are 6 units apart" % ratio
    for name in ("cull off", "unsorted"):
        assert np.max(np.abs(out[name] - out["default"])) < 2e-5


# ----------------------------------------------------------------------------------------------------------------------------
# e. clouds far from the origin: the host's fp64 centring
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows(cf.far_cases(), lambda c: ("grid", "mfma_lean")))
@_stops_at_a_hip_error
def test_far_offset_through_the_registrar(c, engine):
    """Both clouds ~1600 units from the origin (a float32 ulp is 1.2e-4 there, the noise 4e-3): the registrar centres in fp64
    before the float32 upload; px with the centre added back against the oracle on the clouds as generated."""
    plan, init = _plan(c)
    _configure(plan, init, engine)
    _estep(plan, c)
    _assert_engine(plan, engine)
    _compare_points(plan, c, "%s %s" % (cf.case_id(c), engine))


# ----------------------------------------------------------------------------------------------------------------------------
# f. a linear part that is no rotation
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,engine", _rows(cf.affine_cases(), lambda c: ("grid", "mfma_lean")))
@_stops_at_a_hip_error
def test_affine_state(c, engine):
    plan, init = _plan(c)
    _configure(plan, init, engine)
    _estep(plan, c)
    _assert_engine(plan, engine)
    _compare_points(plan, c, "%s %s" % (cf.case_id(c), engine))
