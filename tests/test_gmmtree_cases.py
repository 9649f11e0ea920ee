"""Preconditions of tests/gmmtree_cases.py, held with the fp64 restatement tests/oracle_gmmtree.py alone (no GPU): what
tests/test_gmmtree_stages_gpu.py relies on when it holds gmmtree.hip to a per-node bound of 1e-12.

Every decision the kernels take (first maximum, `den > 1e-15`, `complexity <= lambda_c`, `m0 < lambda_d`) must be far from
its threshold in a case, or two correct fp64 evaluations could take it differently; the one exception is the tie case,
whose tie is exact on purpose."""
import numpy as np
import pytest

import gmmtree_cases as gc
import oracle_gmmtree as og

MIN_GAP = 1.0e-9
DEN_WINDOW = (1.0e-18, 1.0e-12)      # round the `den > 1e-15` cut
DEAD_WINDOW = (0.5e-4, 2.0e-4)       # round the `m0 < lambda_d = 1e-4` rule


def in_window(v, window):
    v = np.asarray(v)
    return int(np.count_nonzero((v >= window[0]) & (v <= window[1])))


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roll", gc.CHUNK_ROLLS)
def test_chunk_case_counts_its_clusters_exactly(roll):
    c = gc.chunk_case(roll)
    sizes = c.extra["sizes"]
    assert sorted(sizes) == sorted(gc.CHUNK_SIZES) and sizes.index(0) == {0: 3, -3: 0, 4: 7}[roll]
    assert {gc.K_CHUNK - 1, gc.K_CHUNK, gc.K_CHUNK + 1, 2 * gc.K_CHUNK, 2 * gc.K_CHUNK + 1, 0, 1} <= set(sizes)
    (m0, _, _), gap = gc.oracle_estep(c)
    assert np.array_equal(m0, np.array(sizes, dtype=np.float64))      # every gamma is exactly 1
    assert np.array_equal(np.bincount(c.extra["label"], minlength=8), sizes)
    assert gap == 1.0


def test_chunk_case_has_an_empty_segment_between_two_of_several_chunks():
    s = gc.chunk_case(0).extra["sizes"]
    assert s[2] > gc.K_CHUNK and s[3] == 0 and s[4] > gc.K_CHUNK


def test_tie_case_gives_both_clusters_to_the_first_twin():
    """The twins share the density, so gamma is exactly 1 / 2 for either and m0[2] = (2049 + 4097) / 2 exactly (a sum of
    halves); the second twin is no point's first maximum."""
    c = gc.tie_case()
    assert np.array_equal(c.nodes[5], c.nodes[2])
    (m0, m1, m2), gap = gc.oracle_estep(c)
    assert gap == 0.0
    assert m0[2] == 0.5 * (gc.CHUNK_SIZES[2] + gc.CHUNK_SIZES[5])
    assert m0[5] == 0.0 and not np.any(m1[5]) and not np.any(m2[5])
    others = [0, 1, 4, 6, 7]
    assert np.array_equal(m0[others], np.array(gc.CHUNK_SIZES, dtype=np.float64)[others]) and m0[3] == 0.0


@pytest.mark.parametrize("tree_level", [1, 2])
def test_far_case_keeps_every_density_off_the_cut(tree_level):
    c = gc.far_case(tree_level)
    zero, faint = c.extra["zero"], c.extra["faint"]
    assert np.array_equal(c.target[zero[:3]], gc.ZERO_POINTS) and np.array_equal(c.target[zero[3:]], gc.dim_points())
    visits = gc.visited_den(gc.moved(c), c.nodes, c.tree_level, c.lambda_c)
    assert len(visits) == tree_level
    for lv, (ai, den) in enumerate(visits):
        assert np.array_equal(ai, np.arange(c.target.shape[0]))       # nothing stops early: every complexity is 1 / 3
        assert np.all(den[zero[:3]] == 0.0) and np.all(den[zero[3:]] < DEN_WINDOW[0])
        assert np.all(den[faint] > 1.0e-12)
        assert in_window(den, DEN_WINDOW) == 0
    root = visits[0][1]
    assert np.all(root[zero[3:]] > 0.0)      # below the cut, but not 0: `den > 0` in place of `den > 1e-15` counts them
    assert np.all(root[faint] < 1.0e-6) and np.all(np.delete(root, np.concatenate([zero, faint])) > 1.0e-7)
    (m0, _, _), gap = gc.oracle_estep(c)
    assert gap >= MIN_GAP
    base, _ = gc.oracle_estep(gc.chunk_case(0))
    if tree_level == 1:   # the zero points add exactly nothing, the faint ones a gamma of 1 each to node 7
        assert np.array_equal(m0[:7], base[0][:7]) and m0[7] == base[0][7] + faint.size
    else:                 # they fall through child 0 of child 0 with weight 0; node 8 holds its own points' mass
        assert not np.any(m0[:8]) and m0[8] > 0.0
        assert 0.0 < m0[8:16].sum() < gc.CHUNK_SIZES[0]               # the chosen child's gamma is below 1 down here


@pytest.mark.parametrize("similarity", [False, True])
def test_octree_case_stops_points_on_every_level(similarity):
    c = gc.octree_case(similarity)
    n = c.target.shape[0]
    assert c.nodes.shape == (4680, 10) and 29000 <= n <= 31000
    (m0, m1, m2), gap = gc.oracle_estep(c)
    hit = [int(np.count_nonzero(m0[og.level(l):og.level(l + 1)] > 0.0)) for l in range(4)]
    assert all(h >= 1 for h in hit) and hit[3] >= 2000, hit
    assert gap >= MIN_GAP
    cplx = og.precompute(c.nodes)[2]
    inner = np.arange(og.level(3))
    assert np.all(np.abs(cplx[inner] - c.lambda_c) >= 1e-6)
    leaves = np.setdiff1d(np.arange(og.level(3), 4680), np.concatenate([c.extra["dead"], c.extra["degen"]]))
    assert np.all(np.abs(cplx[leaves] - c.lambda_c) >= 1e-6)
    assert np.all(cplx[c.extra["flat"]] < c.lambda_c) and abs(cplx[c.extra["flat"][0]] - 0.04 / 2.04) < 1e-12
    for k in ("dead", "degen"):
        assert not np.any(m0[c.extra[k]]) and not np.any(m1[c.extra[k]]) and not np.any(m2[c.extra[k]])
    assert np.all(og.precompute(c.nodes)[0][c.extra["degen"]] == 0.0)
    # the two big leaves hold their clusters (more than one chunk, more than two)
    visits = gc.visited_den(gc.moved(c), c.nodes, 4, c.lambda_c)
    assert [v[0].size for v in visits][0] == n and visits[3][0].size < visits[0][0].size
    for _, den in visits:
        assert in_window(den, DEN_WINDOW) == 0
    assert m0[c.extra["big"][0]] > 0.9 * gc.OCT_BIG[0] and m0[c.extra["big"][1]] > 0.9 * gc.OCT_BIG[1]


def test_octree_similarity_moves_the_tree_with_the_points():
    a, b = gc.octree_case(False), gc.octree_case(True)
    (m0a, _, _), _ = gc.oracle_estep(a)
    (m0b, _, _), _ = gc.oracle_estep(b)
    assert np.array_equal(a.target, b.target) and b.scale == 1.3
    assert np.max(np.abs(m0a - m0b)) <= 1e-9 * np.max(m0a)   # the same geometry: the same masses up to rounding


# ---- B ------------------------------------------------------------------------------------------------------------------
def last_q(info):
    return np.array([q[-1] for q in info["q"]])


@pytest.mark.parametrize("n", gc.STEP_SIZES)
def test_step_case_on_the_oracle(n):
    nodes, info = gc.oracle_build("step", n)
    assert info["iters"] == [1]
    if n in gc.ALL_DEAD_SIZES:
        assert np.array_equal(nodes, np.tile(gc.DEAD_RECORD, (8, 1)))
        assert info["q"][0][0] == n * np.log(1.0e-15)
    else:
        assert np.all(nodes[:, 0] > 0.0)
        assert in_window(info["m0"][0][0], DEAD_WINDOW) == 0
        re_nodes, re_info = gc.oracle_build("step", n, True)
        assert gc.node_error(re_nodes, nodes) <= 1e-13 and gc.q_error(last_q(re_info), last_q(info), n) <= 1e-13


@pytest.mark.parametrize("tree_level", [2, 3])
def test_lopsided_case_on_the_oracle(tree_level):
    c = gc.lopsided_case(tree_level)
    nodes, info = gc.oracle_build("lopsided", tree_level)
    assert info["iters"] == [1] * tree_level
    held = np.bincount(info["cur"][0][0], minlength=8)
    assert held.max() > 2 * gc.K_CHUNK and np.count_nonzero((held > 0) & (held < gc.K_CHUNK)) >= 1 and held.min() == 0
    empty = int(np.argmin(held))
    kids = og.level(1) + 8 * empty + np.arange(8)
    assert np.array_equal(nodes[kids], np.tile(gc.DEAD_RECORD, (8, 1)))
    assert nodes[empty, 0] > 0.0                                       # the parent itself is alive
    for l in range(tree_level):
        assert info["gap"][l][0] >= MIN_GAP
        assert in_window(info["m0"][l][0][og.level(l):og.level(l + 1)], DEAD_WINDOW) == 0
    re_nodes, re_info = gc.oracle_build("lopsided", tree_level, True)
    n = c.points.shape[0]
    assert gc.node_error(re_nodes, nodes) <= 1e-13 and gc.q_error(last_q(re_info), last_q(info), n) <= 1e-13


def test_level4_case_on_the_oracle():
    """The oracle against itself on the points in another order: the rounding noise of this very case, which sets the
    bound of the GPU test (10 times this, at least 1e-12).  Beyond 1e-8 the case would test nothing."""
    nodes, info = gc.oracle_build("level4")
    assert info["iters"] == [2] * 4
    for l in range(4):
        for it in range(2):
            assert info["gap"][l][it] >= MIN_GAP
            assert in_window(info["m0"][l][it][og.level(l):og.level(l + 1)], DEAD_WINDOW) == 0
    node_noise, q_noise = gc.level4_noise()
    print("level-4 build, oracle against itself reordered: nodes %.2e, q %.2e" % (node_noise, q_noise))
    assert node_noise <= 1e-8 and q_noise <= 1e-8
    assert np.count_nonzero(nodes[og.level(3):, 0] > 0.0) >= 400
