"""Seeded cases for the stage tests of GMMTree (probreg_amd/csrc/gmmtree.hip): hand-made trees and targets for the
registration E-step (A), clouds for the build (B).  tests/test_gmmtree_cases.py holds their preconditions with the fp64
restatement tests/oracle_gmmtree.py alone, tests/test_gmmtree_stages_gpu.py runs the kernels on them.  Nothing here needs
a GPU.

A  registration E-step (``set_nodes`` + ``reg_estep``)
    chunk       8 isotropic level-1 nodes on the corners of a cube of edge 4, Sigma = 0.04 I; target clusters of 2047, 2048,
                2049, 0, 4096, 4097, 1 and 300 points (one more / one less than a reduction chunk of 2048 and than two),
                the size list rotated so that the empty node is segment 3, 0 and 7
    tie         chunk, node 5 a bit-identical copy of node 2: the first maximum takes both clusters
    far         chunk (and a level-2 tree over it) plus points whose root-level density is 0 or below 1e-26 and points
                whose density lies between 1e-12 and 1e-6: either side of the `den > 1e-15` cut, never near it
    octree      4680 nodes, one per octant cell of the unit cube down to level 4, flat nodes (complexity 0.0196 <= lambda_c)
                on levels 0..2 stopping the descent early, dead and degenerate leaves, two leaves of 2049 and 4097 points;
                also moved by a similarity, tree and all
B  build (``build`` with lambda_s = 0: every level runs max_iter iterations)
    surface(n)  n = 1, 2, 7 and round the chunk size, one E + M step at level 1
    lopsided    a dense blob, a sparse surface and two outliers: parents of > 4096 and < 2048 points and one that no
                point chooses (its eight children come out dead)
    level 4     surface(6000), two iterations per level

Plain module: no pytest hooks, no fixtures."""
import functools
from collections import namedtuple

import numpy as np

import oracle_gmmtree as og
from probreg_amd import synthetic

K_CHUNK = 2048                      # gmmtree.hip kChunk
DEAD_RECORD = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
LAMBDA_D = 1.0e-4

# nodes (n_nodes, 10), target (n, 3) as handed to set_target, (rot, t, scale) as handed to reg_estep
RegCase = namedtuple("RegCase", ["name", "nodes", "tree_level", "target", "rot", "t", "scale", "lambda_c", "extra"])


def moved(c):
    """The target as the kernel moves it: (scale rot) p + t, fp64."""
    return c.target @ (c.scale * c.rot).T + c.t


def oracle_estep(c):
    """((m0, m1, m2), gap) of the restatement on the moved target."""
    return og.reg_estep(moved(c), c.nodes, c.tree_level, c.lambda_c, return_gap=True)


def visited_den(points, nodes, tree_level, lambda_c):
    """The descent of og.reg_estep once more, returning per level (indices of the points that visit it, their `den` =
    sum of pi_j pdf_j over the eight children before normalisation)."""
    pic, inv, cplx = og.precompute(nodes)
    search = -np.ones(points.shape[0], dtype=np.int64)
    active = np.ones(points.shape[0], dtype=bool)
    out = []
    for _ in range(tree_level):
        ai = np.nonzero(active)[0]
        j = (search[ai, None] + 1) * og.N_NODE + np.arange(og.N_NODE)[None, :]
        g = og._weighted_pdf(points[ai, None, :], nodes[j, 1:4], inv[j], pic[j])
        out.append((ai, g.sum(axis=1)))
        search[ai] = j[np.arange(ai.size), np.argmax(og._normalise(g), axis=1)]
        with np.errstate(invalid="ignore"):
            active[ai[cplx[search[ai]] <= lambda_c]] = False
    return out


# ---- A1 .. A3: the cube of eight nodes ----------------------------------------------------------------------------------
CHUNK_SIZES = (2047, 2048, 2049, 0, 4096, 4097, 1, 300)
CHUNK_ROLLS = (0, -3, 4)            # the empty node as segment 3, 0 and 7
CUBE_SIGMA2 = 0.04
CUBE_LAMBDA_C = 0.01                # isotropic nodes have complexity 1 / 3: the descent never stops early


def cube_nodes():
    nodes = np.zeros((8, 10))
    nodes[:, 0] = 1.0 / 8.0
    for j in range(8):
        nodes[j, 1:4] = [4.0 * (j & 1) - 2.0, 4.0 * ((j >> 1) & 1) - 2.0, 4.0 * ((j >> 2) & 1) - 2.0]
    nodes[:, 4:] = CUBE_SIGMA2 * DEAD_RECORD[4:]
    return nodes


def cube_target(sizes, seed):
    """Clusters mean_j + 0.2 N(0, I) of the given sizes, shuffled; also the cluster of every point."""
    rng = np.random.default_rng(seed)
    mu = cube_nodes()[:, 1:4]
    label = np.repeat(np.arange(8), sizes)
    pts = mu[label] + 0.2 * rng.standard_normal((label.size, 3))
    order = rng.permutation(label.size)
    return pts[order], label[order]


def _identity(name, nodes, tree_level, target, lambda_c, **extra):
    return RegCase(name, nodes, tree_level, target, np.identity(3), np.zeros(3), 1.0, lambda_c, extra)


@functools.lru_cache(maxsize=None)
def chunk_case(roll):
    sizes = tuple(int(s) for s in np.roll(CHUNK_SIZES, roll))
    tgt, label = cube_target(sizes, 31)
    return _identity("chunk%+d" % roll, cube_nodes(), 1, tgt, CUBE_LAMBDA_C, sizes=sizes, label=label)


@functools.lru_cache(maxsize=None)
def tie_case():
    """Node 5 is node 2 once more.  Both have the same density everywhere, so the normalised gamma of either is exactly
    1 / 2 at the points of clusters 2 and 5 (both drawn round the shared mean) and the first of the two takes them."""
    nodes = cube_nodes()
    nodes[5] = nodes[2]
    rng = np.random.default_rng(32)
    label = np.repeat(np.arange(8), CHUNK_SIZES)
    pts = nodes[label, 1:4] + 0.2 * rng.standard_normal((label.size, 3))
    order = rng.permutation(label.size)
    return _identity("tie", nodes, 1, pts[order], CUBE_LAMBDA_C, sizes=CHUNK_SIZES, label=label[order])


ZERO_POINTS = np.array([[1.0e3, 0.0, 0.0], [0.0, -1.0e6, 0.0], [40.0, 40.0, 40.0]])
FAINT_RADII = (1.12, 1.2, 1.28, 1.36, 1.42)   # 0.99 exp(-r^2 / 0.08): 1.5e-7 .. 1.1e-11
DIM_RADII = (2.2, 2.7, 4.0)                   # 5e-27, 1e-40, 1e-87: not 0, but below the cut - `den > 0` would count them


def faint_points():
    """Outwards from node 7 (2, 2, 2) along three directions that leave the cube."""
    dirs = np.array([[3.0, 1.0, 2.0], [1.0, 3.0, 2.5], [2.0, 2.2, 1.0]])   # no two children of node 7 at one distance
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    return np.array([[2.0, 2.0, 2.0] + r * d for d in dirs for r in FAINT_RADII])


def dim_points():
    d = np.array([3.0, 1.0, 2.0]) / np.sqrt(14.0)
    return np.array([[2.0, 2.0, 2.0] + r * d for r in DIM_RADII])


def cube_tree_level2():
    """72 nodes: the cube, and under node j eight children at mean_j + 0.15 (+-1, +-1, +-1) with the same Sigma."""
    nodes = np.zeros((72, 10))
    nodes[:8] = cube_nodes()
    for j in range(8):
        for c in range(8):
            k = 8 + 8 * j + c
            nodes[k, 0] = 1.0 / 64.0
            nodes[k, 1:4] = nodes[j, 1:4] + 0.15 * np.array([2 * (c & 1) - 1, 2 * ((c >> 1) & 1) - 1, 2 * ((c >> 2) & 1) - 1])
            nodes[k, 4:] = CUBE_SIGMA2 * DEAD_RECORD[4:]
    return nodes


@functools.lru_cache(maxsize=None)
def far_case(tree_level):
    base = chunk_case(0)
    zeros = np.concatenate([ZERO_POINTS, dim_points()])
    extra = np.concatenate([zeros, faint_points()])
    pos = np.array([0, 5000, 9000, 2047, 2048, 12000] + list(range(100, 100 + 700 * len(faint_points()), 700)))
    order = np.argsort(pos, kind="stable")
    tgt = np.insert(base.target, pos[order], extra[order], axis=0)   # spread through the cloud, not all in the last block
    where = np.empty_like(pos)
    where[order] = pos[order] + np.arange(pos.size)
    assert np.array_equal(tgt[where], extra)
    nodes = cube_nodes() if tree_level == 1 else cube_tree_level2()
    return _identity("far_L%d" % tree_level, nodes, tree_level, tgt, CUBE_LAMBDA_C, zero=where[:len(zeros)],
                     faint=where[len(zeros):])


def contributing_radius(c):
    """max |coordinate| over the moved points of non-zero weight: the R of the per-node bound without the points that
    contribute exactly 0 (with them R would be 1e6 and the bound on m1, m2 void)."""
    x = moved(c)
    keep = np.ones(x.shape[0], dtype=bool)
    if "zero" in c.extra:
        keep[c.extra["zero"]] = False
    return float(np.max(np.abs(x[keep])))


# ---- A4: the octree -------------------------------------------------------------------------------------------------------
OCT_LAMBDA_C = 0.05
OCT_FLAT = 0.2                      # Sigma_zz = (0.2 s)^2: complexity 0.04 / 2.04 = 0.0196
OCT_BIG = (2049, 4097)
OCT_FLAT_COUNT = (1, 12, 100)       # of 8, 64, 512: about one node in five
OCT_MAX_PER_LEAF = 20


def _octree(seed):
    """Flat nodes: OCT_FLAT_COUNT per level, drawn at random.  Leaves under a flat ancestor get no points of their own
    (they would sit several sigma_z off the flat node, lose to a sibling of it and wander through a subtree that is far
    from them, with densities on either side of 1e-15); every flat node gets three points within a sigma_z of its plane.
    The points of a flat node under a flat ancestor still wander like that (densities down to 1e-147, weight 0): they are
    few, and tests/test_gmmtree_cases.py asserts that none of their densities is near the cut."""
    rng = np.random.default_rng(seed)
    nodes = np.zeros((og.n_nodes(4), 10))
    centre = [np.full((1, 3), 0.5)]
    flat_nodes, under_flat = [], np.zeros(1, dtype=bool)
    for l in range(4):
        edge = 0.5 ** (l + 1)
        k = np.arange(8 ** (l + 1))
        d = k % 8
        bits = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], axis=1)
        ctr = centre[l][k // 8] + (bits - 0.5) * edge
        centre.append(ctr)
        s = 0.3 * edge
        f = np.ones(k.size)
        if l < 3:
            f[rng.choice(k.size, OCT_FLAT_COUNT[l], replace=False)] = OCT_FLAT
        lb = og.level(l)
        nodes[lb + k, 0] = rng.uniform(0.9, 1.1, k.size) / k.size
        nodes[lb + k, 1:4] = ctr
        nodes[lb + k, 4] = nodes[lb + k, 7] = s * s
        nodes[lb + k, 9] = (f * s) ** 2
        flat_nodes.append(lb + k[f != 1.0])
        under_flat = under_flat[k // 8] | (f != 1.0)
    lf = og.level(3)
    free = np.nonzero(~under_flat)[0]
    pick = np.concatenate([rng.permutation(free)[:2], rng.permutation(4096)])
    pick = pick[np.sort(np.unique(pick, return_index=True)[1])]   # the two big leaves first, every leaf once
    big, dead, degen = lf + pick[:2], lf + pick[2:42], lf + pick[42:62]
    nodes[dead] = DEAD_RECORD
    nodes[degen, 9] = 0.0
    # target
    count = rng.integers(0, OCT_MAX_PER_LEAF + 1, 4096)
    count[under_flat] = 0
    count[pick[2:62]] = 0
    count[pick[:2]] = OCT_BIG
    leaf = np.repeat(np.arange(4096), count)
    pts = [centre[4][leaf] + rng.uniform(-0.25, 0.25, (leaf.size, 3)) / 16.0]
    for l in range(3):
        fl = np.repeat(flat_nodes[l] - og.level(l), 3)
        pts.append(centre[l + 1][fl] + rng.uniform(-0.25, 0.25, (fl.size, 3)) * 0.5 ** (l + 1) * np.array([1.0, 1.0, OCT_FLAT]))
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(pts.shape[0])]
    return nodes, pts, dict(dead=dead, degen=degen, big=big, flat=np.concatenate(flat_nodes))


OCT_SIMILARITY = (1.3, (20.0, -10.0), (0.4, -0.7, 0.25))


@functools.lru_cache(maxsize=None)
def octree_case(similarity=False):
    nodes, pts, extra = _octree(41)
    if not similarity:
        return _identity("octree", nodes, 4, pts, OCT_LAMBDA_C, **extra)
    scale, (az, ax), t = OCT_SIMILARITY
    rot, t = synthetic.rot_zx(az, ax), np.array(t)
    out = nodes.copy()
    out[:, 1:4] = nodes[:, 1:4] @ (scale * rot).T + t
    sig = scale * scale * (rot @ nodes[:, 4:][:, og.SYM] @ rot.T)
    out[:, 4:] = sig[:, og.UPPER[0], og.UPPER[1]]
    out[extra["dead"]] = DEAD_RECORD
    return RegCase("octree_sim", out, 4, pts, rot, t, scale, OCT_LAMBDA_C, extra)


# ---- A5: a built level-4 tree -----------------------------------------------------------------------------------------------
BUILT_SOURCE = (20000, 51)          # synthetic.surface(n, seed) the tree is built from
BUILT_TARGET = (30000, 52)
BUILT_MAX_ITER = 3
BUILT_LAMBDA_C = 0.01


def built_source():
    return synthetic.surface(*BUILT_SOURCE)


def built_target():
    return synthetic.surface(*BUILT_TARGET) @ synthetic.rot_zx(10.0, 5.0).T


# ---- B: builds ------------------------------------------------------------------------------------------------------------
BuildCase = namedtuple("BuildCase", ["name", "points", "tree_level", "idx", "max_iter"])
STEP_SIZES = (1, 2, 7, 2047, 2048, 2049, 4097)
ALL_DEAD_SIZES = (1, 2)


def step_case(n):
    return BuildCase("step%d" % n, synthetic.surface(n, 61), 1, og.init_indices(n, 1, 0), 1)


LOPSIDED_N = (7000, 5000)           # blob, surface; and two outliers
LOPSIDED_IDX_SEED = {2: 8, 3: 5}   # of seeds 1..8 the ones that leave a level-0 child without points


@functools.lru_cache(maxsize=None)
def lopsided_points():
    """A blob of 7000 points (sd 0.05) at (0.9, 0.1, 0), surface(5000) and, as the last two points, outliers 40 and 60
    away from the cloud's mean along one line."""
    rng = np.random.default_rng(62)
    cloud = np.concatenate([np.array([0.9, 0.1, 0.0]) + 0.05 * rng.standard_normal((LOPSIDED_N[0], 3)),
                            synthetic.surface(LOPSIDED_N[1], 63)])
    cloud = cloud[rng.permutation(cloud.shape[0])]
    m = cloud.mean(axis=0)
    u = np.array([0.0, 0.6, 0.8])
    return np.concatenate([cloud, [m + 40.0 * u, m + 60.0 * u]])


def lopsided_case(tree_level, seed=None):
    """Leaves from the cloud, one leaf under level-0 child 1 from the nearer outlier.  With the seeds above the blob's
    child is the first choice of > 8000 points, most of the others of a few hundred and one of none (asserted in
    tests/test_gmmtree_cases.py, with the gap of every E-step)."""
    pts = lopsided_points()
    n = pts.shape[0]
    idx = og.init_indices(n - 2, tree_level, LOPSIDED_IDX_SEED[tree_level] if seed is None else seed)
    idx[8 ** (tree_level - 1)] = n - 2
    return BuildCase("lopsided_L%d" % tree_level, pts, tree_level, idx, 1)


LEVEL4 = (6000, 71)


def level4_case():
    n, seed = LEVEL4
    return BuildCase("level4", synthetic.surface(n, seed), 4, og.init_indices(n, 4, 0), 2)


@functools.lru_cache(maxsize=None)
def oracle_build(name, tree_level=None, reorder=False):
    """og.build(lambda_s = 0, trace) of a build case by name; `reorder`: on the points in another order with the leaf
    indices remapped - the same problem, other rounding."""
    c = {"level4": level4_case, "lopsided": lambda: lopsided_case(tree_level), "step": lambda: step_case(tree_level)}[name]()
    pts, idx = c.points, c.idx
    if reorder:
        perm = np.random.default_rng(7).permutation(pts.shape[0])
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        pts, idx = pts[perm], inv[idx]
    return og.build(pts, c.tree_level, idx, 0.0, LAMBDA_D, c.max_iter, trace=True)


def node_error(a, b):
    """The largest error of the records a against b in units of the node's own scale (the form of
    test_gmmtree_gpu.assert_nodes_close): |pi|, |mu| / scale, |Sigma| / scale^2."""
    mu_b, sig_b = b[:, 1:4], b[:, 4:]
    scale = np.max(np.abs(mu_b), axis=1) + np.sqrt(np.max(np.abs(sig_b), axis=1))
    return max(float(np.max(np.abs(a[:, 0] - b[:, 0]))), float(np.max(np.abs(a[:, 1:4] - mu_b) / scale[:, None])),
               float(np.max(np.abs(a[:, 4:] - sig_b) / (scale ** 2)[:, None])))


def q_error(q, ref, n):
    return float(np.max(np.abs(np.asarray(q) - np.asarray(ref)) / np.maximum(np.abs(ref), n)))


def _last_q(info):
    return np.array([q[-1] for q in info["q"]])


def level4_noise():
    """(node error, q error) of the oracle's level-4 build against itself on the reordered points."""
    nodes, info = oracle_build("level4")
    re_nodes, re_info = oracle_build("level4", None, True)
    return node_error(re_nodes, nodes), q_error(_last_q(re_info), _last_q(info), LEVEL4[0])


def level4_bounds():
    """10 times the noise (one reordering is a single sample of it), at least 1e-12."""
    return tuple(max(10.0 * v, 1.0e-12) for v in level4_noise())
