"""Exact k-NN lists and radius counts on the GPU (IcpPlan.knn / radius_count, csrc/grid_search.hip: k_icp_knn, k_icp_radius_count)
against their restatement (tests/oracle_knn.py).

index (int32), d2 and count are compared byte for byte: a list is the k smallest (d2, n) of exactly rounded d2, which does not
depend on the grid, the levels or the order of the visits.
"""
import functools

import numpy as np
import pytest

import oracle_icp as oi
import oracle_knn as ok
from probreg_amd import synthetic

pytestmark = pytest.mark.gpu

EDGES = (None, 0.01, 0.3, 8.0)  # the cloud's own choice, many cells (hashed), a few cells, a single cell
RADII = (0.02, 0.15, np.inf)
KS = (2, 8, 20, 64)


def _icp():
    from probreg_amd import icp
    return icp


class _Plan(object):
    def __init__(self, src, tgt, pose=None, cell_edge=None):
        self.plan = _icp().IcpPlan()
        self.src, self.tgt, self.pose, self.cell_edge = src, tgt, pose, cell_edge

    def __enter__(self):
        self.plan.set_target(self.tgt, cell_edge=self.cell_edge)
        self.plan.set_source(self.src)
        if self.pose is not None:
            self.plan.set_pose(self.pose)
        return self.plan

    def __exit__(self, *exc):
        self.plan.close()


def _same(got, ref):
    return (got[0].dtype == np.int32 and got[2].dtype == np.int32 and got[0].shape == ref[0].shape
            and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
            and got[2].tobytes() == ref[2].tobytes())


def _no_index_twice(idx):
    s = np.sort(idx, axis=1)
    return not np.any((s[:, 1:] == s[:, :-1]) & (s[:, 1:] >= 0))


def _cut(ref, k):
    """The restatement's lists for a smaller k: the first k entries of every list."""
    return np.ascontiguousarray(ref[0][:, :k]), np.ascontiguousarray(ref[1][:, :k]), np.minimum(ref[2], k).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _grid_case(variant):
    src, tgt, (rot, t, _) = synthetic.rigid_pair(1500, m=1200, seed=3)
    src, tgt = src.copy(), tgt.copy()
    if variant == "outlier":
        tgt[700] = (1.0e6, -1.0e6, 1.0e6)
    if variant == "far":
        src[:50, 0] += 3.0 * (tgt[:, 0].max() - tgt[:, 0].min())
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt, oi.pose12(rot, t)


def _reference(variant, at_true_pose, r):
    """The restatement's lists of a grid case with k = 64, computed once."""
    def make():
        src, tgt, true_pose = _grid_case(variant)
        return ok.knn(oi.moved(src, true_pose if at_true_pose else oi.IDENTITY), tgt, 64, r)
    return ok.cached(("grid", variant, at_true_pose, r), make)


CASES = [(v, p) for v in ("plain", "outlier", "far") for p in (False, True)]


# ------------------------------------------------------------------------------------------------------------ 1: k = 1
@pytest.mark.parametrize("variant, at_true_pose", CASES)
def test_k1_equals_the_existing_search(variant, at_true_pose):
    src, tgt, true_pose = _grid_case(variant)
    pose = true_pose if at_true_pose else oi.IDENTITY
    for edge in EDGES:
        with _Plan(src, tgt, pose, edge) as plan:
            for r in RADII:
                plan.search(r)
                idx, d2 = plan.matches()
                got = plan.knn(1, r)
                what = (variant, at_true_pose, r, edge)
                assert got.index.shape == (1200, 1) and got.index.dtype == np.int32 and got.count.dtype == np.int32, what
                assert got.index[:, 0].tobytes() == idx.tobytes() and got.d2[:, 0].tobytes() == d2.tobytes(), what
                assert np.array_equal(got.count, (idx >= 0).astype(np.int32)), what
                assert _same(got, _cut(_reference(variant, at_true_pose, r), 1)), what


# ------------------------------------------------------------------------------------------------------------ 2: larger k
@pytest.mark.parametrize("variant, at_true_pose", CASES)
def test_lists_do_not_depend_on_the_grid(variant, at_true_pose):
    """Also trap 1: a point that is seen again - on the next level after a hand-over, through a second cell of a hashed
    bucket (edge 0.01) - must not enter a list twice."""
    src, tgt, true_pose = _grid_case(variant)
    pose = true_pose if at_true_pose else oi.IDENTITY
    for edge in EDGES:
        with _Plan(src, tgt, pose, edge) as plan:
            for r in RADII:
                ref = _reference(variant, at_true_pose, r)
                if variant == "far":
                    assert np.all(ref[2][:50] == 0) if np.isfinite(r) else np.all(ref[2][:50] == 64)
                for k in KS:
                    got = plan.knn(k, r)
                    what = (variant, at_true_pose, r, edge, k)
                    assert _no_index_twice(got.index), what
                    assert _same(got, _cut(ref, k)), what


# ---------------------------------------------------------------------------------------------------------------- 3: ties
def test_ties_between_copies_go_to_the_smaller_index():
    base = synthetic.surface(400, 21)
    cloud = np.ascontiguousarray(np.tile(base, (8, 1)))
    ref = ok.knn(cloud, cloud, 20)
    for edge in (None, 0.05, 8.0):
        with _Plan(cloud, cloud, None, edge) as plan:
            got = plan.knn(20)
        assert np.all(got.d2[:, :8] == 0.0)
        first = (np.arange(3200) % 400)[:, None] + 400 * np.arange(8)[None, :]
        assert np.array_equal(got.index[:, :8], first)  # the copies in ascending index, the point itself where it falls
        assert _no_index_twice(got.index) and _same(got, ref), edge


def test_ties_on_a_quantised_cloud():
    cloud = np.ascontiguousarray(np.round(synthetic.surface(1500, 21), 1))
    q = np.ascontiguousarray(np.round(synthetic.surface(300, 22), 1))
    for k, r in ((8, np.inf), (20, 0.25), (64, np.inf)):
        ref = ok.knn(q, cloud, k, r)
        assert np.any(ref[1][:, 1:] == ref[1][:, :-1])  # there are ties to decide
        for edge in (None, 0.01, 1.0):
            with _Plan(q, cloud, None, edge) as plan:
                got = plan.knn(k, r)
            assert _no_index_twice(got.index) and _same(got, ref), (k, r, edge)


# --------------------------------------------------------------------------------------------------------- 4: short lists
@pytest.mark.parametrize("n", [1, 5])
def test_a_cloud_smaller_than_k(n):
    cloud = synthetic.surface(n, 2)
    q = np.concatenate([cloud, synthetic.surface(70, 3)])
    with _Plan(q, cloud) as plan:
        got = plan.knn(64)
    assert np.all(got.count == n) and np.all(got.index[:, n:] == -1) and np.all(np.isposinf(got.d2[:, n:]))
    assert np.all(got.index[:, :n] >= 0) and np.all(np.isfinite(got.d2[:, :n]))
    assert _same(got, ok.knn(q, cloud, 64))


def test_a_radius_that_cuts_lists_short():
    cloud, q = synthetic.surface(1500, 4), synthetic.surface(400, 5)
    r, k = 0.12, 20
    ref = ok.knn(q, cloud, k, r)
    assert ref[2].min() < 3 and ref[2].max() == k and np.sum((ref[2] > 0) & (ref[2] < k)) > 50  # lengths between 0 and k
    for edge in EDGES:
        with _Plan(q, cloud, None, edge) as plan:
            got = plan.knn(k, r)
        assert _same(got, ref), edge


# ----------------------------------------------------------------------------------------------------- 5: the radius edge
def test_radius_edge_is_inside_and_one_ulp_out_is_not():
    origin, r = np.zeros((1, 3)), 5.0 / 16.0
    y = np.array([[3.0, 4.0, 0.0]]) / 16.0
    out = y.copy()
    out[0, 1] = np.nextafter(out[0, 1], np.inf)
    for edge in (None, 0.1, 1.0):
        with _Plan(origin, y, None, edge) as plan:
            got = plan.knn(4, r)
            assert got.index[0].tolist() == [0, -1, -1, -1] and got.d2[0, 0] == r * r and got.count[0] == 1
            assert plan.radius_count(r).tolist() == [1]
        with _Plan(origin, out, None, edge) as plan:
            got = plan.knn(4, r)
            assert got.index[0].tolist() == [-1] * 4 and np.all(np.isposinf(got.d2)) and got.count[0] == 0
            assert plan.radius_count(r).tolist() == [0]


# ------------------------------------------------------------------------------------------ 6: a far k-th neighbour (trap 2)
def test_kth_neighbour_far_beyond_three_shells():
    """A list that is not full yet must not stop on the distance of its last entry: a query in the cluster of 12 has to
    collect 8 points of the cluster 50 extents away."""
    rng = np.random.default_rng(11)
    small = rng.uniform(-0.5, 0.5, (12, 3))
    large = rng.uniform(-0.5, 0.5, (300, 3)) + np.array([50.0, 0.0, 0.0])
    lone = rng.uniform(-60.0, 60.0, (10, 3)) + np.array([0.0, 200.0, 0.0])
    cloud = np.ascontiguousarray(np.concatenate([small, large, lone]))
    q = np.ascontiguousarray(np.concatenate([small[:6], small[:6] + 0.01, large[:4], lone[:2]]))
    ref = ok.knn(q, cloud, 20)
    assert np.all(np.sum((ref[0][:12] >= 12) & (ref[0][:12] < 312), axis=1) == 8)
    for edge in (None, 0.02, 0.5, 300.0):
        with _Plan(q, cloud, None, edge) as plan:
            got = plan.knn(20)
        assert np.all(got.count == 20) and _no_index_twice(got.index) and _same(got, ref), edge


# ---------------------------------------------------------------------------------------- 7: repeatability, radius counts
def test_two_runs_give_the_same_bytes():
    src, tgt, pose = _grid_case("plain")
    runs = []
    for _ in range(2):
        with _Plan(src, tgt, pose) as plan:
            runs.append((plan.knn(20, 0.15), plan.radius_count(0.15)))
    assert _same(runs[0][0], runs[1][0]) and runs[0][1].tobytes() == runs[1][1].tobytes()


@pytest.mark.parametrize("variant, at_true_pose", CASES)
def test_radius_count_equals_the_restatement(variant, at_true_pose):
    src, tgt, true_pose = _grid_case(variant)
    pose = true_pose if at_true_pose else oi.IDENTITY
    q = oi.moved(src, pose)
    for r in (0.02, 0.15, 0.7, 1.0e7):
        ref = ok.radius_count(q, tgt, r)
        if r in RADII:  # the lists' lengths are the counts, cut to k
            assert np.array_equal(np.minimum(ref, 64), _reference(variant, at_true_pose, r)[2])
        for edge in EDGES:
            with _Plan(src, tgt, pose, edge) as plan:
                got = plan.radius_count(r)
            assert got.dtype == np.int32 and got.tobytes() == ref.tobytes(), (variant, at_true_pose, r, edge)


def test_module_level_calls():
    icp = _icp()
    cloud, q = synthetic.surface(700, 8), synthetic.surface(90, 9)
    res = icp.knn_search(q, cloud, 8, max_distance=0.3)
    assert isinstance(res, icp.KnnResult) and _same(res, ok.knn(q, cloud, 8, 0.3))
    assert _same(icp.knn_search(cloud, cloud, 3), ok.knn(cloud, cloud, 3))
    assert icp.radius_count(q, cloud, 0.3).tobytes() == ok.radius_count(q, cloud, 0.3).tobytes()
    nn = icp.nearest_neighbour(q, cloud)
    one = icp.knn_search(q, cloud, 1)
    assert one.index[:, 0].tobytes() == nn[0].tobytes() and one.d2[:, 0].tobytes() == nn[1].tobytes()
