"""GMMTree's kernels (probreg_amd/csrc/gmmtree.hip) stage by stage on the MI355X, through GmmTreePlan, against the fp64
restatement tests/oracle_gmmtree.py on the cases of tests/gmmtree_cases.py (their preconditions: tests/test_gmmtree_cases.py).

A  registration E-step, per node.  For node j with the oracle's m0_j and R = max |coordinate| of the moved points that
   carry weight: |m0 - ref| <= 1e-12 m0_j, |m1 - ref| <= 1e-12 m0_j R, |m2 - ref| <= 1e-12 m0_j R^2, and a node whose m0_j
   is exactly 0 comes back as ten exact zeros.  A node's sum has at most 4097 non-negative summands here: reordering
   them costs at most k eps = 4.6e-13 of the sum of their absolute values, each summand's own error (the exponent's
   rounding, the 8-term normalisation) is below 1e-14.  The bound is per node because the chunk and segment tables are:
   an error in a node of one point beside a node of 4000 is invisible relative to the largest entry.
B  build with lambda_s = 0 (every level runs max_iter iterations on both sides): nodes in units of the node's own scale
   and q, dq per level as |q - ref| <= tol max(|ref|, n), tol = 1e-12 (the same k eps) for one E + M step per level.
   The level-4 build runs two iterations on four levels and carries rounding forward, so its bound is measured, not
   derived: 10 times the oracle's difference against itself on the points in another order, at least 1e-12.
C  a handle that has held larger problems and another level returns the bytes of a fresh handle.

Measured on the MI355X (each test prints its figure before it asserts):
  A, worst error / per-node bound   chunk edges 0.002 (all three rotations), first maximum 0.002, far points 0.002 (level
     1) and 0.001 (level 2), octree 0.003, octree under the similarity 0.002, the built level-4 tree 0.673
  B, one step at level 1            nodes <= 4.1e-15, q and dq <= 4.2e-16 (n = 1, 2: exact, all eight children dead)
     lopsided, levels 2 and 3       nodes 8.0e-15 / 1.2e-14, q and dq 2.4e-14 / 4.6e-14
     (the oracle against itself on reordered points: nodes <= 1.1e-14, q <= 4.8e-14 - the 1e-12 stands)
     level-4 build                  oracle against itself reordered: nodes 1.48e-10, q 1.91e-12, hence the bounds
                                    1.48e-9 and 1.91e-11; observed nodes 1.35e-10, q 1.49e-12, dq 3.30e-12
  C  equal bytes
The built tree is the one case near its bound, and not by the sums: its nodes come from a thin surface, their
covariances reach a condition number of 2e5, and the quadratic form d^T Sigma^-1 d of a point in such a node's plane is
only good to cond eps in any fp64 evaluation (the kernel's cofactor inverse and the restatement's LU inverse differ by
that much from each other and from an extended-precision inverse).  The hand-made trees have cond <= 25.
"""
import numpy as np
import pytest

import gmmtree_cases as gc
import oracle_gmmtree as og

pytestmark = pytest.mark.gpu

A_TOL = 1.0e-12
B_TOL = 1.0e-12


@pytest.fixture()
def plan():
    from probreg_amd.gmmtree import GmmTreePlan

    p = GmmTreePlan()
    yield p
    p.close()


def gpu_estep(plan, c):
    plan.set_nodes(c.nodes, c.tree_level)
    plan.set_target(c.target)
    return plan.reg_estep(c.rot, c.t, c.scale, c.lambda_c, with_m2=True)


def per_node_ratio(m01, m2, ref, radius, what):
    """Largest error in units of the per-node bound; nodes of zero mass must be exact zeros."""
    m0, m1, m2r = ref
    m2r = m2r[:, og.UPPER[0], og.UPPER[1]]
    empty = m0 == 0.0
    assert not np.any(m01[empty]) and not np.any(m2[empty]), what
    assert np.array_equal(m01[:, 0] == 0.0, empty), what
    w = m0[~empty]
    ratio = max(float(np.max(np.abs(m01[~empty, 0] - w) / (A_TOL * w))),
                float(np.max(np.abs(m01[~empty, 1:] - m1[~empty]) / (A_TOL * w * radius)[:, None])),
                float(np.max(np.abs(m2[~empty] - m2r[~empty]) / (A_TOL * w * radius ** 2)[:, None])))
    print("%s: worst error / per-node bound = %.3f (%d nodes with mass, R = %.3g)" % (what, ratio, w.size, radius))
    return ratio


def check_estep(plan, c, radius=None):
    m01, m2 = gpu_estep(plan, c)
    ref, _ = gc.oracle_estep(c)
    radius = float(np.max(np.abs(gc.moved(c)))) if radius is None else radius
    assert per_node_ratio(m01, m2, ref, radius, c.name) <= 1.0
    return m01, m2, ref


# ---- A ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("roll", gc.CHUNK_ROLLS)
def test_chunk_edges(plan, roll):
    c = gc.chunk_case(roll)
    m01, _, _ = check_estep(plan, c)
    sizes = np.array(c.extra["sizes"], dtype=np.float64)    # an independent count
    assert np.all(np.abs(m01[:, 0] - sizes) <= 1e-12 * sizes)


def test_first_maximum(plan):
    c = gc.tie_case()
    m01, m2, _ = check_estep(plan, c)
    assert m01[2, 0] == 0.5 * (gc.CHUNK_SIZES[2] + gc.CHUNK_SIZES[5])
    assert not np.any(m01[5]) and not np.any(m2[5])         # `>=` in the argmax would hand node 5 everything


@pytest.mark.parametrize("tree_level", [1, 2])
def test_far_points(plan, tree_level):
    c = gc.far_case(tree_level)
    m01, _, ref = check_estep(plan, c, gc.contributing_radius(c))
    if tree_level == 2:
        assert ref[0][8] > 0.0 and abs(m01[8, 0] - ref[0][8]) <= A_TOL * ref[0][8]


@pytest.mark.parametrize("similarity", [False, True])
def test_level4_octree(plan, similarity):
    check_estep(plan, gc.octree_case(similarity))


def test_built_level4_tree(plan):
    """The GPU's own level-4 tree on both sides.  The preconditions need its nodes, so they are asserted here."""
    src, tgt = gc.built_source(), gc.built_target()
    idx = og.init_indices(src.shape[0], 4, 0)
    iters, _, _ = plan.build(src, 4, idx, 0.001, gc.LAMBDA_D, gc.BUILT_MAX_ITER)
    assert list(iters) == [gc.BUILT_MAX_ITER] * 4
    nodes = plan.get_nodes()
    plan.set_target(tgt)
    m01, m2 = plan.reg_estep(np.identity(3), np.zeros(3), 1.0, gc.BUILT_LAMBDA_C, with_m2=True)
    ref, gap = og.reg_estep(tgt, nodes, 4, gc.BUILT_LAMBDA_C, return_gap=True)
    cplx = og.precompute(nodes)[2]
    hit = [int(np.count_nonzero(ref[0][og.level(l):og.level(l + 1)] > 0.0)) for l in range(4)]
    print("built level-4 tree: gap %.2e, complexity margin %.2e, nodes with mass per level %s"
          % (gap, np.nanmin(np.abs(cplx - gc.BUILT_LAMBDA_C)), hit))
    assert gap >= 1e-9 and np.nanmin(np.abs(cplx - gc.BUILT_LAMBDA_C)) >= 1e-6 and hit[3] > 0
    assert per_node_ratio(m01, m2, ref, float(np.max(np.abs(tgt))), "built level-4 tree") <= 1.0


# ---- B ------------------------------------------------------------------------------------------------------------------
def check_build(plan, c, ref_nodes, info, node_tol, q_tol):
    iters, q, dq = plan.build(c.points, c.tree_level, c.idx, 0.0, gc.LAMBDA_D, c.max_iter)
    nodes = plan.get_nodes()
    n = c.points.shape[0]
    assert list(iters) == [c.max_iter] * c.tree_level == info["iters"]
    q_ref = np.array([v[-1] for v in info["q"]])
    dq_ref = np.array([abs(v[-1] - (v[-2] if len(v) > 1 else 0.0)) for v in info["q"]])
    errs = gc.node_error(nodes, ref_nodes), gc.q_error(q, q_ref, n), gc.q_error(dq, dq_ref, n)
    print("%s: node error %.2e (bound %.2e), q error %.2e, dq error %.2e (bound %.2e)"
          % (c.name, errs[0], node_tol, errs[1], errs[2], q_tol))
    assert np.array_equal(nodes[:, 0] == 0.0, ref_nodes[:, 0] == 0.0)     # the same nodes are dead
    assert errs[0] <= node_tol and errs[1] <= q_tol and errs[2] <= q_tol
    return nodes, q


@pytest.mark.parametrize("n", gc.STEP_SIZES)
def test_one_step_at_level_1(plan, n):
    c = gc.step_case(n)
    ref_nodes, info = gc.oracle_build("step", n)
    if n in gc.ALL_DEAD_SIZES:
        nodes, q = check_build(plan, c, ref_nodes, info, 0.0, 1e-14)   # |q| = 34.5 n > n: relative
        assert np.array_equal(nodes, np.tile(gc.DEAD_RECORD, (8, 1)))
        assert abs(q[0] - n * np.log(1.0e-15)) <= 1e-14 * abs(q[0])
    else:
        check_build(plan, c, ref_nodes, info, B_TOL, B_TOL)


@pytest.mark.parametrize("tree_level", [2, 3])
def test_one_step_per_level_on_a_lopsided_cloud(plan, tree_level):
    ref_nodes, info = gc.oracle_build("lopsided", tree_level)
    check_build(plan, gc.lopsided_case(tree_level), ref_nodes, info, B_TOL, B_TOL)


def test_level4_build(plan):
    ref_nodes, info = gc.oracle_build("level4")
    noise = gc.level4_noise()
    node_tol, q_tol = gc.level4_bounds()
    print("level-4 build: oracle against itself reordered: nodes %.2e, q %.2e" % noise)
    check_build(plan, gc.level4_case(), ref_nodes, info, node_tol, q_tol)


# ---- C ------------------------------------------------------------------------------------------------------------------
def _reuse_steps():
    def estep(c):
        return lambda p: b"".join(a.tobytes() for a in gpu_estep(p, c))

    def build(p):
        x = gc.synthetic.surface(5000, 81)
        out = p.build(x, 2, og.init_indices(5000, 2, 0), 0.001, gc.LAMBDA_D, 5)
        return b"".join(np.asarray(a).tobytes() for a in out) + p.get_nodes().tobytes()

    return [("octree", estep(gc.octree_case(False))), ("chunk", estep(gc.chunk_case(0))), ("build L2", build),
            ("octree again", estep(gc.octree_case(False)))]


def test_reused_handle_gives_a_fresh_handles_bytes(plan):
    """GPU against GPU on purpose: the determinism claim of gmmtree.hip with workspaces that held larger problems and a
    tree reallocated for another level."""
    from probreg_amd.gmmtree import GmmTreePlan

    for what, step in _reuse_steps():
        fresh = GmmTreePlan()
        try:
            want = step(fresh)
        finally:
            fresh.close()
        assert step(plan) == want, what
