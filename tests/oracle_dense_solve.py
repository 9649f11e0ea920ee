"""Two independent float64 host solves of the systems behind the dense non-rigid M-step and the BCPD solve, and the
yardstick they define (TEST INFRASTRUCTURE for tests/test_dense_solve_gpu.py and tests/test_oracle_dense_solve.py).

Non-rigid M-step (reference cpd.py:296-297, with correspondence priors :391-396), from the float32 kernel matrix the
plan holds, cast to float64:
    (diag(d) G + c I) W = b,   d = p1 [+ f p1_tilde],   b = px - p1 y [+ f (px_tilde - p1_tilde y)],
    c = lmd sigma2_prev,       f = sigma2_prev / alpha
  solve 1   LAPACK LU on the system as it stands (``np.linalg.solve``) - the reference the GPU is compared with
  solve 2   the push-through SPD form  W = (b - D^1/2 S^-1 D^1/2 G b) / c,  S = c I + D^1/2 G D^1/2,  with scipy's
            Cholesky, plus two steps of float64 iterative refinement on the original system when priors are set

BCPD (reference bcpd.py:123-133):
  solve 1   the explicit form  Sigma = inv(lmd inv(G) + cfac diag(nu))
  solve 2   Woodbury           Sigma = (G - B^T S^-1 B) / lmd,  B = D^1/2 G,  S = (lmd / cfac) I + D^1/2 G D^1/2  (LU)

The yardstick of a quantity is the relative max-norm disagreement of the two host answers: the round-off two correct
float64 solvers leave under the conditioning of THAT case.  A third solver is held to ``bound(y, m)``:

    8 * max(y, m * 2^-53)   relative to the largest entry of solve 1

  8       the difference of two answers is the sum of two round-off errors under the same conditioning; 8 leaves room
          for another summation order (k-permuted matrix-core chains, blocked panels) and stays below one decimal digit
  floor   m * 2^-53 is the plain bound of a dot product of length m.  The host BLAS beats it by blocking, a correct
          chain of fused multiply-adds need not.
Nothing here looks at the code under test.
"""
import functools
from collections import namedtuple

import numpy as np
import scipy.linalg

from oracle import bcpd_numpy as bo
from oracle import cpd_numpy as co

FACTOR = 8.0
UNIT = 2.0 ** -53
BETA = 2.0
LMD = 2.0
SIGMA2_LATE = 1e-4   # deep in the late regime of a registration: cond(S) ~ 2e7
N_PAIRS = 25

# caps on the yardstick itself (tests/test_oracle_dense_solve.py): a case whose two host solves disagree by more proves
# nothing about a third solver and must be replaced, not loosened
Y_CAP = 1e-8
Y_CAP_TINY_ALPHA = 1e-7


def bound(y, m):
    return FACTOR * max(y, m * UNIT)


def rel_max(a, b):
    """max |a - b| relative to the largest entry of b (the reference)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


# ---- cases --------------------------------------------------------------------------------------------------------
# state: "init" = sigma2_prev from the closed-form initialiser, "late" = SIGMA2_LATE.  zero_rows: every tenth source
# point loses its support (p1 = 0 and px = 0 exactly).  dim = 2 drops the cloud's last coordinate.  alpha: trust in
# N_PAIRS seeded correspondence pairs (None: no priors).
NonrigidCase = namedtuple("NonrigidCase", ["m", "state", "zero_rows", "dim", "alpha"])
BcpdCase = namedtuple("BcpdCase", ["m", "cfac"])


def _nr(m, state, zero_rows=False, dim=3, alpha=None):
    return NonrigidCase(m, state, zero_rows, dim, alpha)


# every row of the look-ahead schedule table, both ragged roundings (100 -> 104 of 128, 121 -> 128), the exact block and
# panel multiples, and one real row in the last block (1025)
SCHEDULE_SIZES = (100, 121, 128, 300, 512, 777, 1024, 1025, 1100, 1700)
DENSE_CASES = [_nr(m, s) for m in SCHEDULE_SIZES for s in ("init", "late")]
ZERO_ROW_CASES = [_nr(m, s, zero_rows=True) for m in (300, 1100) for s in ("init", "late")]
ORDER_CASE = _nr(1100, "late")           # run with and without the plan's own sort of the source
PLANAR_CASE = _nr(300, "late", dim=2)
CONSTRAINED_CASES = [_nr(m, "init", alpha=a) for m in (300, 1100) for a in (1e-2, 1e-8)]
NONRIGID_CASES = DENSE_CASES + ZERO_ROW_CASES + [PLANAR_CASE] + CONSTRAINED_CASES   # (ORDER_CASE is one of DENSE_CASES)
# 2300: the K-deep left update (17 block rows and more) and the update inside a second panel (18 and more)
BCPD_CASES = [BcpdCase(m, c) for m in (100, 1100, 2300) for c in (37.5, 4e4)]


def case_id(case):
    if isinstance(case, BcpdCase):
        return "m%d-cfac%g" % case
    tags = ["m%d" % case.m, case.state]
    if case.zero_rows:
        tags.append("zerorows")
    if case.dim != 3:
        tags.append("d%d" % case.dim)
    if case.alpha is not None:
        tags.append("alpha%g" % case.alpha)
    return "-".join(tags)


NonrigidInputs = namedtuple("NonrigidInputs", ["y", "x", "pt1", "p1", "px", "sigma2_prev", "lmd", "beta", "alpha",
                                               "p1_tilde", "px_tilde"])


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def nonrigid_inputs(case):
    """The clouds (float32 values, as the plan stores them) and the host oracle's E-step at W = 0."""
    from probreg_amd import synthetic

    m = case.m
    y, x = synthetic.nonrigid_pair(m + 150, m=m, seed=m)
    y, x = np.ascontiguousarray(y[:, :case.dim]), np.ascontiguousarray(x[:, :case.dim])
    sigma2 = co.squared_kernel_sum_closed_form(y, x) if case.state == "init" else SIGMA2_LATE
    es = co.expectation_step(y, x, sigma2, 0.0)
    p1, px = es.p1.copy(), es.px.copy()
    if case.zero_rows:
        p1[3::10] = 0.0
        px[3::10] = 0.0
    p1t = pxt = None
    if case.alpha is not None:
        rng = np.random.default_rng(m)
        i_src = rng.choice(m, N_PAIRS, replace=False)
        i_tgt = rng.choice(x.shape[0], N_PAIRS, replace=False)
        p1t, pxt = np.zeros(m), np.zeros((m, case.dim))
        np.add.at(p1t, i_src, 1.0)                      # row sums of the 0-1 matrix of cpd.py:370-374 ...
        np.add.at(pxt, i_src, x[i_tgt])                 # ... and its product with the target
    _frozen(y, x, es.pt1, p1, px, p1t, pxt)
    return NonrigidInputs(y, x, es.pt1, p1, px, float(sigma2), LMD, BETA, case.alpha, p1t, pxt)


def kernel_f32(inp):
    """The reference's float32 G (transformation.py:91-99) - what a plan's get_g() returns to 1.2e-7."""
    return co.rbf_kernel(inp.y, inp.y, inp.beta).astype(np.float64)


def kernel_exact(inp):
    """G in float64 from the float32 points: what the low-rank factor reproduces."""
    d = inp.y[:, None, :] - inp.y[None, :, :]
    return np.exp(-np.einsum("mnd,mnd->mn", d, d) / (2.0 * inp.beta))


# ---- the non-rigid system and its two solves ------------------------------------------------------------------------
def nonrigid_system(inp):
    """(d, c, b) of (diag(d) G + c I) W = b."""
    d = inp.p1.copy()
    b = inp.px - inp.p1[:, None] * inp.y                             # cpd.py:296
    if inp.alpha is not None:
        f = inp.sigma2_prev / inp.alpha
        d = d + f * inp.p1_tilde                                     # cpd.py:391-393
        b = b + f * (inp.px_tilde - inp.p1_tilde[:, None] * inp.y)   # cpd.py:394-395
    return d, inp.lmd * inp.sigma2_prev, b


def solve_lu(g, d, c, b):
    return np.linalg.solve(d[:, None] * g + c * np.identity(len(d)), b)


def solve_push_through(g, d, c, b, nrefine):
    sd = np.sqrt(d)
    s = sd[:, None] * g * sd[None, :]
    s[np.diag_indices_from(s)] += c
    factor = scipy.linalg.cho_factor(s, lower=True)

    def apply(rhs):
        return (rhs - sd[:, None] * scipy.linalg.cho_solve(factor, sd[:, None] * (g @ rhs))) / c

    w = apply(b)
    for _ in range(nrefine):
        w = w + apply(b - (d[:, None] * (g @ w) + c * w))
    return w


def sigma2_of(inp, disp):
    """cpd.py:298-302 with T = y + G W; the three traces are summed in extended precision so that the reference's own
    summation error stays out of the comparison (they cancel by two to four digits)."""
    ld = np.longdouble
    t = inp.y.astype(ld) + disp.astype(ld)
    x = inp.x.astype(ld)
    tr_xp1x = np.sum(inp.pt1.astype(ld) * np.sum(x * x, axis=1))
    tr_pxt = np.sum(inp.px.astype(ld) * t)
    tr_tpt = np.sum(inp.p1.astype(ld) * np.sum(t * t, axis=1))
    return float((tr_xp1x - 2 * tr_pxt + tr_tpt) / (np.sum(inp.p1.astype(ld)) * inp.y.shape[1]))


NonrigidReference = namedtuple("NonrigidReference", ["w", "disp", "sigma2", "y_w", "y_disp", "y_sigma2", "y_w_unrefined"])


def nonrigid_reference(inp, g):
    """Solve 1 and the yardsticks (disagreement with solve 2) of W, G W and sigma2.  ``y_w_unrefined``: how far the
    push-through form is from LU WITHOUT its refinement steps (equal to y_w when no priors are set)."""
    d, c, b = nonrigid_system(inp)
    w1 = solve_lu(g, d, c, b)
    nrefine = 2 if inp.alpha is not None else 0
    w2 = solve_push_through(g, d, c, b, nrefine)
    w0 = solve_push_through(g, d, c, b, 0) if nrefine else w2
    g1, g2 = g @ w1, g @ w2
    s1, s2 = sigma2_of(inp, g1), sigma2_of(inp, g2)
    _frozen(w1, g1)
    return NonrigidReference(w1, g1, s1, rel_max(w2, w1), rel_max(g2, g1), abs(s2 - s1) / abs(s1), rel_max(w0, w1))


@functools.lru_cache(maxsize=None)
def nonrigid_reference_f32(case):
    """The reference of a case on the oracle's float32 G (the CPU test; the GPU test takes the plan's own matrix)."""
    inp = nonrigid_inputs(case)
    return nonrigid_reference(inp, kernel_f32(inp))


# ---- BCPD -------------------------------------------------------------------------------------------------------------
BcpdInputs = namedtuple("BcpdInputs", ["src", "nu", "resid", "lmd", "cfac"])
BcpdReference = namedtuple("BcpdReference", ["sigma_diag", "v_hat", "y_sigma_diag", "y_v_hat"])


@functools.lru_cache(maxsize=None)
def bcpd_inputs(case):
    """The set-up of test_bcpd_gpu.py::test_solve_matches_dense_inverse with the box scaled by m^(1/3) (same point
    density at every size) and a twelfth of the points without support."""
    m = case.m
    rng = np.random.default_rng(m)
    half = 12.0 * (m / 777.0) ** (1.0 / 3.0)
    src = rng.uniform(-half, half, (m, 3)).astype(np.float32).astype(np.float64)
    nu = rng.uniform(0.0, 2.0, m)
    nu[rng.choice(m, m // 12, replace=False)] = 0.0
    resid = rng.normal(0.0, 0.3, (m, 3))
    _frozen(src, nu, resid)
    return BcpdInputs(src, nu, resid, LMD, case.cfac)


def bcpd_kernel(inp):
    return bo.inverse_multiquadric_kernel(inp.src, inp.src).astype(np.float64)


def bcpd_explicit(g, inp):
    sigma = np.linalg.inv(inp.lmd * np.linalg.inv(g) + inp.cfac * np.diag(inp.nu))      # bcpd.py:123-125
    return np.diag(sigma).copy(), inp.cfac * sigma @ (inp.nu[:, None] * inp.resid)     # bcpd.py:126


def bcpd_woodbury(g, inp):
    sd = np.sqrt(inp.nu)
    bmat = sd[:, None] * g
    s = bmat * sd[None, :]
    s[np.diag_indices_from(s)] += inp.lmd / inp.cfac
    sigma = (g - bmat.T @ np.linalg.solve(s, bmat)) / inp.lmd
    return np.diag(sigma).copy(), inp.cfac * sigma @ (inp.nu[:, None] * inp.resid)


@functools.lru_cache(maxsize=None)
def bcpd_reference(case):
    inp = bcpd_inputs(case)
    g = bcpd_kernel(inp)
    sd1, v1 = bcpd_explicit(g, inp)
    sd2, v2 = bcpd_woodbury(g, inp)
    _frozen(sd1, v1)
    return BcpdReference(sd1, v1, rel_max(sd2, sd1), rel_max(v2, v1))
