"""Cases for the FilterReg plan's lattice choice (tests/test_filterreg_routes_cases.py on the host,
tests/test_filterreg_routes_gpu.py on the GPU).

The reference builds the blurred lattice and rebuilds without the blur if it has more than N * alpha vertices
(filterreg.py:90-91).  prg_fr_estep gives the same answer by several routes that depend on the previous E-step's answer
(prg_fr_last_route); the alpha script below walks one plan through all of them with the clouds and sigma2 held still, so that
every step can be compared with the oracle's E-step of the same inputs.
"""
import numpy as np

from oracle import filterreg_numpy as fo
from oracle import permutohedral as po
from probreg_amd import synthetic

SIGMA2 = 0.05
SEED = 8
SAMPLE_PERIOD = 16      # the plan decides on every 16th point first
SAMPLED_FROM = 4096     # ... when M + N is at least this

# (name, M, N, dim) of the alpha-script cases
SCRIPT_CASES = [
    ("tot4095", 1500, 2595, 3),     # one short of the sampling threshold: nothing is sampled
    ("tot4096", 1500, 2596, 3),     # 0 mod 16
    ("tot4097", 1500, 2597, 3),     # 1 mod 16
    ("tot4111", 1500, 2611, 3),     # 15 mod 16
    ("m4095", 4095, 2500, 3),       # source kept in the caller's order
    ("m4096", 4096, 2500, 3),       # source Morton-sorted, outputs through the permutation
    ("lopsided_n", 16, 4200, 3),
    ("lopsided_m", 4200, 16, 3),    # N * 0.015 < 1: the threshold is 0 vertices
    ("flat", 1500, 2596, 2),        # 2-D: m1 is a two-channel filter, which the reference runs through seqCompute
]
SCRIPT_IDS = [c[0] for c in SCRIPT_CASES]


def clouds(m, n, dim=3, seed=SEED):
    """(source [m, dim], target [n, dim]) float64; the 2-D case is the first two columns of the 3-D one."""
    src, tgt, _ = synthetic.filterreg_pair(n, m=m, seed=seed)
    return np.ascontiguousarray(src[:, :dim]), np.ascontiguousarray(tgt[:, :dim])


def features(src, tgt, sigma2):
    """The lattice's points as the reference forms them (filterreg.py:84-85), in the caller's order."""
    sigma = np.sqrt(sigma2)
    return np.r_[src / sigma, tgt / sigma]


def lattice_sizes(src, tgt, sigma2):
    """(blurred, non-blurred, blurred over every 16th row of the caller-order cloud) vertex counts of the oracle's lattice."""
    f = features(src, tgt, sigma2)
    return (po.Lattice(f, True).lattice_size, po.Lattice(f, False).lattice_size,
            po.Lattice(f[::SAMPLE_PERIOD], True).lattice_size)


def boundary_alpha(s_b, n):
    """The smallest double a with n * a >= s_b in fp64: at a the blurred lattice of s_b vertices is kept, one step below
    it is not.  s_b / n is that number or a neighbour of it (the product rounds once more)."""
    a = float(s_b) / float(n)
    while n * a < s_b:
        a = float(np.nextafter(a, np.inf))
    while n * float(np.nextafter(a, 0.0)) >= s_b:
        a = float(np.nextafter(a, 0.0))
    return a


def step_alphas(src, tgt, sigma2):
    """The alpha of each of the eight steps (expected_script tells what each one has to do)."""
    n = tgt.shape[0]
    s_b = po.Lattice(features(src, tgt, sigma2), True).lattice_size
    a_eq = boundary_alpha(s_b, n)
    return [a_eq, float(np.nextafter(a_eq, 0.0)), 0.015, (s_b - 0.5) / n, a_eq, 0.0, -1.0, 1.0e9]


def expected_script(tot):
    """(with_blur, route, lattice builds, sampled) per step of the script on a plan fresh from set_state (which makes the
    first E-step try the blurred lattice first).  Below 4096 points nothing is sampled: the side proof of step 3 becomes a
    whole blurred build that is rejected, and step 4 needs two builds, not three.
    Steps 7 and 8 have no threshold a vertex count could be compared with (negative, or >= 2e9): the blurred lattice is
    built whole, whatever the previous step did, which prg_fr_last_route counts as blurred-first."""
    sampled = tot >= SAMPLED_FROM
    return [
        (True, 1, 1, 0),
        (False, 2, 2, 0),
        (False, 3, 1, 1) if sampled else (False, 6, 2, 0),
        (False, 6, 3, 1) if sampled else (False, 6, 2, 0),
        (True, 5, 2, 1) if sampled else (True, 5, 1, 0),
        (False, 2, 2, 0),
        (False, 2, 2, 0),
        (True, 1, 1, 0),
    ]


def oracle_step(src, tgt, rot, t, sigma2, alpha=0.015, w=0.0, objective_type="pt2pt", target_normals=None):
    """One EM iteration of the oracle from (rot, t, sigma2): returns (t_source, EstepResult, (lattice size, with_blur),
    MstepResult) with the sigma2 update on."""
    ts = np.dot(src, np.asarray(rot).T) + np.asarray(t)
    info = []
    es = fo.expectation_step(ts, tgt, tgt, sigma2, True, alpha=alpha, info=info,
                             target_normals=target_normals if objective_type == "pt2pl" else None)
    ms = fo.maximization_step(ts, tgt, es, np.asarray(rot), np.asarray(t), sigma2, w=w, objective_type=objective_type)
    return ts, es, info[0], ms


# ---- table sizing (one plan, M = 8000, N = 12000) -------------------------------------------------------------------
TABLE_M, TABLE_N = 8000, 12000
# (sigma2, alpha) per step; alpha 0 rejects every blurred lattice, 1e9 keeps it.  The plan gets each sigma2 through set_state,
# which makes the E-step build the blurred lattice first: with alpha 0 both kinds are built, with 1e9 the blurred one alone.
TABLE_STEPS = [
    (0.5, 0.0),      # tiny lattices of both kinds: the next tables of both kinds are the smallest (65536 slots)
    (1.0e-5, 0.0),   # > 32768 vertices of both kinds: more than half of 65536, both builds are retried at full capacity
    (0.5, 1.0e9),    # blurred and tiny again, table sized from the large one
    (1.0e-4, 1.0e9), # blurred and > 32768 vertices in a table sized from a tiny one: the neighbour look-ups need the retry's mask
    (0.5, 1.0e9),
    (0.5, 1.0e9),    # smallest table again, over the slots the large lattices left behind (older generations)
    (0.5, 0.0),
    (0.5, 0.0),      # the same for the non-blurred kind
]
TABLE_MIN_SLOTS = 65536


def table_capacity(tot, dim):
    """Slots of a plan's hash table: the power of two that holds 2 * tot * (dim + 1) entries."""
    cap = 1
    while cap < 2 * tot * (dim + 1):
        cap <<= 1
    return cap


def table_attempts(prev_size, size, cap):
    """Attempts of a build of `size` vertices after one of `prev_size` of the same kind: the table is sized for 8 x the
    previous lattice (65536 slots at least, the whole table at most or when there was none) and retried whole when it comes
    out more than half full."""
    used = cap
    if prev_size > 0:
        used = TABLE_MIN_SLOTS
        while used < 8 * prev_size:
            used <<= 1
        used = min(used, cap)
    return 1 if 2 * size <= used else 2


def table_script(sizes, n, tot, dim=3):
    """Per step of TABLE_STEPS (with_blur, lattice size, route, builds, attempts of the last build), from
    sizes[sigma2] = (blurred, non-blurred) vertex counts."""
    cap = table_capacity(tot, dim)
    prev = [0, 0]
    out = []
    for sigma2, alpha in TABLE_STEPS:
        s_b, s_nb = sizes[sigma2]
        att = table_attempts(prev[1], s_b, cap)
        prev[1] = s_b
        if s_b > n * alpha:
            att = table_attempts(prev[0], s_nb, cap)
            prev[0] = s_nb
            out.append((False, s_nb, 2, 2, att))
        else:
            out.append((True, s_b, 1, 1, att))
    return out
