"""The weighted (BCPD) E-step's cases on the cloud families of tests/cloud_families.py: per-source weights
a_m = alpha_m exp(-s^2 D Sigma_mm / 2 sigma2) (reference: probreg/bcpd.py:56-61) on the cube, the 10 : 1 : 1 box, the two blobs and the
target blob the source lacks, in the dense / mid / late states.  tests/test_weighted_cases.py holds their preconditions with the fp64
oracle alone, tests/test_weighted_estep_gpu.py runs every engine that carries the weights on them.  Nothing here needs a GPU.

Sizes: M = 2100, N = 1900 (and swapped) - no multiple of 32 / 128 / 256 / 512, several blocks on either side; weighted plans never
reach the matrix cores, so nothing as large as the unweighted families' clouds is needed.

Weight sets
    default   alpha ~ Dirichlet(1.5), Sigma_mm = U(0, 1) 12 (2 sigma2 / D): the exponent of the second factor lies in [0, 12] in
              every state, ln a_m spans ~17 (test_weighted_cases.py holds <= 20), so q_m = -2 sigma2 (ln a_m - max) reaches 40 sigma2
    uniform   alpha = 1 / M, Sigma_mm = 0: every q_m is 0 and the outlier ratio is M / N - the plain CPD E-step
    dead      default, but every 7th source point has an exponent of 2000: its a_m is exactly 0 in fp64

Plain module: no pytest hooks, no fixtures."""
from collections import namedtuple

import numpy as np

import cloud_families as cf
from oracle import bcpd_numpy as bo

FAMILIES = cf.FAMILIES
STATES = ("dense", "mid", "late")
M_DEFAULT, N_DEFAULT = 2100, 1900
WEIGHT_SEED = 23
DEAD_STRIDE, DEAD_EXPONENT = 7, 2000.0
TILE_SIZES = ((3, 700), (700, 4), (33, 31), (129, 127), (513, 255))

# base: the cloud_families.Case (family, state, w, sizes, dim) - the plain CPD case of the same clouds and state; wset: the weight set
WCase = namedtuple("WCase", ["base", "wset"])


def outlier_weight(family, state):
    """The families' rule: 0.1, but 0 for `lopsided` past its dense state (the blob without a partner would take the mass)."""
    return 0.0 if family == "lopsided" and state != "dense" else 0.1


def wcase(family, state, m=M_DEFAULT, n=N_DEFAULT, dim=3, wset="default", w=None):
    assert state in STATES and wset in ("default", "uniform", "dead")
    return WCase(cf.case(family, state, outlier_weight(family, state) if w is None else w, m=m, n=n, dim=dim), wset)


def weights(m, dim, sigma2, seed=WEIGHT_SEED):
    """(alpha [m], sigma_diag [m]) of the default set."""
    g = np.random.default_rng(seed)
    alpha = g.dirichlet(np.full(m, 1.5))
    sigma_diag = g.random(m) * 12.0 * 2.0 * sigma2 / dim
    return alpha, sigma_diag


def dead_rows(m):
    return np.arange(0, m, DEAD_STRIDE)


def grid_cases():
    return [wcase(f, s) for f in FAMILIES for s in STATES]


def two_d_cases():
    return [wcase("clusters", s, dim=2) for s in STATES]


def swapped_cases():
    return [wcase(f, "mid", m=N_DEFAULT, n=M_DEFAULT) for f in FAMILIES]


def tile_cases():
    """`volume mid` at sizes around the tile edges (fewer points than a group of 32, one more / one less than a block of 128 and a
    chunk of 512), with the uniform term and without it (w = 0: every column of P sums to one whatever the pads hold)."""
    return [wcase("volume", "mid", m=m, n=n, w=w) for m, n in TILE_SIZES for w in (0.1, 0.0)]


def special_cases():
    return [wcase("clusters", "mid", wset="dead"), wcase("clusters", "mid", wset="uniform")]


def all_cases():
    return grid_cases() + two_d_cases() + swapped_cases() + tile_cases() + special_cases()


def case_id(c):
    b = c.base
    tag = "%s-%s-w%g" % (b.family, b.state, b.w)
    if (b.m, b.n) != (M_DEFAULT, N_DEFAULT):
        tag += "-%dx%d" % (b.m, b.n)
    if b.dim != 3:
        tag += "-2d"
    if c.wset != "default":
        tag += "-" + c.wset
    return tag


def case_setup(c):
    """cloud_families.case_setup of the clouds and the state (shared by every weight set of a cloud pair; read only)."""
    return cf.case_setup(c.base)


_WEIGHTS, _ORACLE = {}, {}


def case_weights(c):
    """(alpha [m], sigma_diag [m]) of a case, as bcpd._estep_on_plan and the oracle take them (cached; read only)."""
    if c not in _WEIGHTS:
        b = c.base
        st = case_setup(c)["st_c"]
        if c.wset == "uniform":
            alpha, sd = np.full(b.m, 1.0 / b.m), np.zeros(b.m)
        else:
            alpha, sd = weights(b.m, b.dim, st.sigma2)
            if c.wset == "dead":
                sd[dead_rows(b.m)] = DEAD_EXPONENT * 2.0 * st.sigma2 / (st.scale ** 2 * b.dim)
        _WEIGHTS[c] = (alpha, sd)
    return _WEIGHTS[c]


def log_weights(c):
    """ln a_m in fp64 (bcpd.py:56-61 without the factors common to every m)."""
    b = c.base
    st = case_setup(c)["st_c"]
    alpha, sd = case_weights(c)
    return np.log(alpha) - st.scale ** 2 * b.dim / (2.0 * st.sigma2) * sd


def plan_clouds(c):
    """(transformed source, target) in fp64 as the oracles see them: the state applied in fp64 to the centred float32 source, and the
    centred float32 target - the values a plan holds."""
    s = case_setup(c)
    return cf.transformed(s["st_c"], s["s32"].astype(np.float64)), s["t32"].astype(np.float64)


def oracle_at(c, z, x):
    """The fp64 numpy oracle's weighted E-step (oracle.bcpd_numpy.expectation_step, reference bcpd.py:53-72) of a case's weights and
    state at explicit clouds."""
    st = case_setup(c)["st_c"]
    alpha, sd = case_weights(c)
    return bo.expectation_step(z, x, st.scale, alpha, sd, st.sigma2, c.base.w)


def oracle_estep(c):
    """... of the case itself (cached; callers must not modify it): EstepResult(nu_d, nu, n_p, px, x_hat)."""
    if c not in _ORACLE:
        _ORACLE[c] = oracle_at(c, *plan_clouds(c))
    return _ORACLE[c]


def oracle_plain(c):
    """The plain CPD E-step of the same clouds, state and w (cloud_families.oracle_estep: the fp64 C oracle; cached)."""
    return cf.oracle_estep(c.base)
