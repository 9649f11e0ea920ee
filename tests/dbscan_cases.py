"""The clouds of the DBSCAN tests (tests/test_oracle_dbscan.py on the host, tests/test_dbscan_gpu.py on the GPU) and their
restatement results, computed once per process (oracle_dbscan.cached).  ``synthetic`` is handed in: this file does not
import the product."""
import numpy as np

import oracle_dbscan as od

PARAMS = ((0.25, 8), (0.15, 10))  # (eps, min_points) of the scene
SCENE_OBJECTS = (900, 600, 300)   # rows of a, b, c before the permutation; then 80 outliers


def scene(synthetic):
    """(cloud (1880, 3), origin (1880,): the object 0 / 1 / 2 of every row, -1 for an outlier)."""
    def make():
        a = synthetic.surface(900, 11)
        b = 0.8 * synthetic.surface(600, 12) + np.array([3.0, 0.2, 0.1])
        c = 0.6 * synthetic.surface(300, 13) + np.array([0.3, 2.4, 0.9])
        rng = np.random.default_rng(0)
        out = rng.uniform((-1.6, -1.0, -0.8), (4.2, 3.2, 1.6), (80, 3))
        cloud = np.concatenate([a, b, c, out], axis=0)
        origin = np.concatenate([np.full(900, 0), np.full(600, 1), np.full(300, 2), np.full(80, -1)])
        perm = rng.permutation(cloud.shape[0])
        return np.ascontiguousarray(cloud[perm]), origin[perm]
    return od.cached("dbscan_scene", make)


def scene_ref(synthetic, eps, min_points):
    return od.cached(("dbscan_scene", eps, min_points), lambda: od.dbscan(scene(synthetic)[0], eps, min_points))


def chain():
    """3000 points 0.09 apart along a shallow sine, permuted: one long component."""
    def make():
        t = np.arange(3000, dtype=np.float64)
        pts = np.stack([0.09 * t, 0.01 * np.sin(0.09 * t), np.zeros(3000)], axis=1)
        return np.ascontiguousarray(pts[np.random.default_rng(5).permutation(3000)])
    return od.cached("dbscan_chain", make)


def tie_cloud(left_first=False):
    """(cloud (9, 3), eps = 1, min_points = 4): two groups of four points at x = +-(1, 1.25, 1.5, 1.75) and the origin last.
    Every coordinate and every d2 is exact.  A group spans 0.75, so each of its points has the four of its group within eps
    and is core; the groups are 2 apart, so they are two clusters.  The origin has d2 == eps eps to the two points at
    x = +-1 and to nothing else: three neighbours with itself, not core, a border point at the same distance from both
    clusters.  It goes with the smaller core index: index 0, the group that comes first (x > 0 unless ``left_first``)."""
    x = 1.0 + 0.25 * np.arange(4)
    right = np.stack([x, np.zeros(4), np.zeros(4)], axis=1)
    groups = [-right, right] if left_first else [right, -right]
    return np.ascontiguousarray(np.concatenate(groups + [np.zeros((1, 3))], axis=0)), 1.0, 4
