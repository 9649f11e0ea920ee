"""Preconditions of tests/filterreg_routes.py, held with the oracle alone (no GPU): the inputs of
tests/test_filterreg_routes_gpu.py can reach what they are meant to reach.

The GPU test's own route assertions are the real check; what is asserted here is that the alpha script sits exactly on the
reference's `lattice_size > n * alpha` decision (filterreg.py:90), that a sixteenth of a cloud can neither prove nor miss
what the script wants it to, and that the table-sizing script crosses the half-full mark of the smallest table."""
import numpy as np
import pytest

import filterreg_routes as fr
from oracle import filterreg_numpy as fo


@pytest.fixture(scope="module", params=fr.SCRIPT_CASES, ids=fr.SCRIPT_IDS)
def case(request):
    name, m, n, dim = request.param
    src, tgt = fr.clouds(m, n, dim)
    assert src.shape == (m, dim) and tgt.shape == (n, dim)
    return name, src, tgt, fr.lattice_sizes(src, tgt, fr.SIGMA2)


def test_case_sizes_sit_where_the_plan_changes_path():
    tots = {name: m + n for name, m, n, _ in fr.SCRIPT_CASES}
    assert tots["tot4095"] == fr.SAMPLED_FROM - 1 and tots["tot4096"] == fr.SAMPLED_FROM
    assert [tots[k] % fr.SAMPLE_PERIOD for k in ("tot4096", "tot4097", "tot4111")] == [0, 1, 15]
    ms = {name: m for name, m, _, _ in fr.SCRIPT_CASES}
    assert ms["m4095"] == 4095 and ms["m4096"] == 4096      # the source is Morton-sorted from 4096 points on
    assert all(m + n <= 20000 for _, m, n, _ in fr.SCRIPT_CASES)


def test_boundary_alpha_is_the_last_double_that_keeps_the_blurred_lattice(case):
    name, src, tgt, (s_b, s_nb, _) = case
    n = tgt.shape[0]
    a_eq = fr.boundary_alpha(s_b, n)
    below = float(np.nextafter(a_eq, 0.0))
    assert abs(a_eq - s_b / n) <= 4.0 * np.spacing(s_b / n)
    assert n * a_eq >= s_b and n * below < s_b
    assert s_nb < s_b
    for alpha, want in ((a_eq, (s_b, True)), (below, (s_nb, False))):
        info = []
        fo.expectation_step(src, tgt, tgt, fr.SIGMA2, True, alpha=alpha, info=info)
        assert info == [want], (name, alpha)


def test_script_alphas_decide_as_the_script_expects(case):
    name, src, tgt, (s_b, s_nb, _) = case
    n = tgt.shape[0]
    alphas = fr.step_alphas(src, tgt, fr.SIGMA2)
    want = fr.expected_script(src.shape[0] + n)
    assert len(alphas) == len(want) == 8
    assert [not s_b > n * a for a in alphas] == [w[0] for w in want]    # the reference's decision, filterreg.py:90
    # step 4: the threshold the plan compares a vertex count with is S_b - 1, one vertex short
    assert np.floor(n * alphas[3]) == s_b - 1
    # steps 7 and 8: no such threshold (negative / >= 2e9, also for the 16-point target)
    assert n * alphas[6] < 0.0 and n * alphas[7] >= 2.0e9


def test_a_sixteenth_of_the_cloud_proves_step_3_and_not_step_4(case):
    """Blurred vertices of every 16th row of the caller-order cloud: more than N * 0.015 (the sample proves that the blurred
    lattice is too large), fewer than S_b - 1 (it proves nothing about thresholds S_b - 1 and S_b).  The plan samples its own
    Morton order, so this is a plausibility window."""
    name, src, tgt, (s_b, _, s_16) = case
    assert tgt.shape[0] * 0.015 < s_16 < s_b - 1, name


def test_pt2pl_case_reaches_both_of_its_steps():
    from probreg_amd import synthetic

    src, tgt, nrm, _ = synthetic.pt2pl_pair(2596, m=1500, seed=9)
    s_b, s_nb, s_16 = fr.lattice_sizes(src, tgt, fr.SIGMA2)
    assert src.shape[0] + tgt.shape[0] == fr.SAMPLED_FROM and nrm.shape == tgt.shape
    assert tgt.shape[0] * 0.015 < s_16 < s_b - 1 and s_nb < s_b


def test_table_script_crosses_half_of_the_smallest_table():
    src, tgt = fr.clouds(fr.TABLE_M, fr.TABLE_N)
    tot = fr.TABLE_M + fr.TABLE_N
    assert tot <= 20000
    sizes = {s2: fr.lattice_sizes(src, tgt, s2)[:2] for s2 in sorted({s for s, _ in fr.TABLE_STEPS})}
    half = fr.TABLE_MIN_SLOTS // 2
    assert 8 * max(sizes[0.5]) <= fr.TABLE_MIN_SLOTS            # a tiny lattice asks for the smallest table
    assert min(sizes[1.0e-5]) > half and sizes[1.0e-4][0] > half
    assert fr.table_capacity(tot, 3) > fr.TABLE_MIN_SLOTS       # ... which is smaller than the whole one
    script = fr.table_script(sizes, fr.TABLE_N, tot)
    assert [s[0] for s in script] == [a > 0.0 for _, a in fr.TABLE_STEPS]
    assert [s[4] for s in script] == [1, 2, 1, 2, 1, 1, 1, 1]
    # the builds of steps 5 and 7 are sized from a large lattice, those of steps 6 and 8 from a tiny one again
    cap = fr.table_capacity(tot, 3)
    assert fr.table_attempts(sizes[1.0e-4][0], 0, cap) == fr.table_attempts(0, 0, cap) == 1
    assert 8 * sizes[1.0e-4][0] > fr.TABLE_MIN_SLOTS and 8 * sizes[1.0e-5][1] > fr.TABLE_MIN_SLOTS


@pytest.mark.parametrize("m,n", [(3000, 3500), (6000, 9000)])
def test_trajectory_clouds_and_the_routes_they_can_reach(m, n):
    """The oracle's own 10 iterations: at M = 3000, N = 3500 the blurred lattice has twice the N * 0.015 = 52.5 vertices
    already at the first sigma2 and grows from there, so no E-step of that trajectory can keep it (route 1); the larger pair
    starts below its threshold and crosses it."""
    src, tgt = fr.clouds(m, n)
    sigma2 = max(float(fo.squared_kernel_sum_f32(src, tgt)), 1.0e-4)
    rot, t = np.identity(3), np.zeros(3)
    blur = []
    for _ in range(10):
        _, _, info, ms = fr.oracle_step(src, tgt, rot, t, sigma2, w=0.05)
        blur.append(info[1])
        rot, t, sigma2 = ms.rot, ms.t, max(ms.sigma2, 1.0e-4)
    if (m, n) == (3000, 3500):
        assert not any(blur)
    else:
        k = blur.index(False)
        assert k >= 1 and not any(blur[k:]) and len(blur) - k >= 2      # kept, then rejected, then at least one side proof
