"""The clouds of the plane-segmentation tests (tests/test_oracle_plane.py, test_plane_host.py, test_plane_gpu.py) and the
restatement's results on them, computed once per process and never written to.

  table   N = 2248 (two full scoring pieces and a partial one): 1500 points of a table top tilted by rot_zx(25, 12) with
          uniform noise +-0.004 across it, two objects (0.5 surface(400, 11), 0.4 surface(250, 12)) standing 0.8 and 0.9
          above it, 98 uniform outliers of which two lie within tau = 0.01 of the table; all permuted.  Analytic normals ride
          along (the outliers' are random directions).
  room    N = 3072 (exactly three pieces): a floor of 1500, walls of 900 and 500 points (noise +-0.004 each), 172 outliers,
          all turned by rot_zx(40, 20) and permuted.
  exact clouds: two 5 x 5 integer lattices, a point exactly at tau, a collinear cloud, a cloud on the 2^-20 grid and its shift.
"""
import functools

import numpy as np

import oracle_plane as op

TAU = 0.01
N_HYP = 1000
NOISE = 0.004
TABLE_ROT_DEG = (25.0, 12.0)
ROOM_ROT_DEG = (40.0, 20.0)
TABLE_N, TABLE_PLANE_N = 2248, 1500
ROOM_N, ROOM_SIZES = 3072, (1500, 900, 500)
ROOM_MIN_INLIERS = 100
NORMAL_ANGLE = np.radians(20.0)
EIGEN_BOUND = 1.0e-13   # |n_gpu - n_ref| <= EIGEN_BOUND / gap: the bound of the FPFH normal tests
SHIFT_EXACT = np.array([2.0 ** 20, -2.0 ** 20, 2.0 ** 20])


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def table_scene():
    """(points (2248, 3), normals (2248, 3), is_table (2248,) bool, the table's unit normal (3,))."""
    from probreg_amd import synthetic

    rng = np.random.default_rng(2025)
    rot = synthetic.rot_zx(*TABLE_ROT_DEG)
    top = np.stack([rng.uniform(-1.0, 1.0, TABLE_PLANE_N), rng.uniform(-1.0, 1.0, TABLE_PLANE_N),
                    rng.uniform(-NOISE, NOISE, TABLE_PLANE_N)], axis=1)
    top_n = np.tile([0.0, 0.0, 1.0], (TABLE_PLANE_N, 1))
    o1, n1 = synthetic.surface_with_normals(400, 11)
    o2, n2 = synthetic.surface_with_normals(250, 12)
    o1 = 0.5 * o1 + np.array([-0.4, 0.3, 0.8])
    o2 = 0.4 * o2 + np.array([0.45, -0.35, 0.9])
    out = np.stack([rng.uniform(-1.2, 1.2, 98), rng.uniform(-1.2, 1.2, 98), rng.uniform(-0.5, 1.5, 98)], axis=1)
    out_n = rng.normal(size=(98, 3))
    out_n /= np.linalg.norm(out_n, axis=1)[:, None]
    pts = np.concatenate([top, o1, o2, out]) @ rot.T + np.array([0.3, -0.2, 0.5])
    nrm = np.concatenate([top_n, n1, n2, out_n]) @ rot.T
    is_table = np.arange(TABLE_N) < TABLE_PLANE_N
    perm = rng.permutation(TABLE_N)
    return _freeze(np.ascontiguousarray(pts[perm]), np.ascontiguousarray(nrm[perm]), is_table[perm],
                   np.ascontiguousarray(rot[:, 2]))


@functools.lru_cache(maxsize=None)
def room_scene():
    """(points (3072, 3), part (3072,) int: 0 floor, 1 and 2 the walls, -1 outliers, the three unit normals (3, 3))."""
    from probreg_amd import synthetic

    rng = np.random.default_rng(3030)
    rot = synthetic.rot_zx(*ROOM_ROT_DEG)
    nf, n1, n2 = ROOM_SIZES
    floor = np.stack([rng.uniform(0.0, 2.0, nf), rng.uniform(0.0, 1.6, nf), rng.uniform(-NOISE, NOISE, nf)], axis=1)
    wall1 = np.stack([rng.uniform(0.0, 2.0, n1), rng.uniform(-NOISE, NOISE, n1), rng.uniform(0.05, 1.2, n1)], axis=1)
    wall2 = np.stack([rng.uniform(-NOISE, NOISE, n2), rng.uniform(0.05, 1.6, n2), rng.uniform(0.05, 1.2, n2)], axis=1)
    n_out = ROOM_N - nf - n1 - n2
    out = np.stack([rng.uniform(0.1, 2.0, n_out), rng.uniform(0.1, 1.6, n_out), rng.uniform(0.1, 1.2, n_out)], axis=1)
    pts = np.concatenate([floor, wall1, wall2, out]) @ rot.T
    part = np.concatenate([np.zeros(nf), np.ones(n1), np.full(n2, 2), np.full(n_out, -1)]).astype(np.int64)
    perm = rng.permutation(ROOM_N)
    normals = np.stack([rot[:, 2], rot[:, 1], rot[:, 0]])
    return _freeze(np.ascontiguousarray(pts[perm]), part[perm], normals)


@functools.lru_cache(maxsize=None)
def lattices():
    """Two 5 x 5 integer lattices on z = 0 and z = 1 (50 points), z = 0 first."""
    g = np.stack(np.meshgrid(np.arange(5.0), np.arange(5.0), indexing="ij"), axis=-1).reshape(25, 2)
    return _freeze(np.ascontiguousarray(np.concatenate([np.concatenate([g, np.full((25, 1), z)], axis=1) for z in (0.0, 1.0)])))


@functools.lru_cache(maxsize=None)
def quarter_cloud():
    """A 4 x 4 lattice on z = 0 and one point at z = 0.25: with tau = 0.25 it is exactly at the threshold of z = 0."""
    g = np.stack(np.meshgrid(np.arange(4.0), np.arange(4.0), indexing="ij"), axis=-1).reshape(16, 2)
    return _freeze(np.ascontiguousarray(np.concatenate([np.concatenate([g, np.zeros((16, 1))], axis=1), [[1.5, 2.5, 0.25]]])))


@functools.lru_cache(maxsize=None)
def collinear_cloud():
    t = np.arange(40.0)
    return _freeze(np.ascontiguousarray(np.stack([t, 2.0 * t, -t], axis=1)))


@functools.lru_cache(maxsize=None)
def grid_cloud(n=300):
    """A slab (|z| <= 0.02 around a tilted plane) and outliers, n points, every coordinate a multiple of 2^-20 and below 4 in
    size: the shift by SHIFT_EXACT is exact, and so is every difference of two shifted coordinates."""
    rng = np.random.default_rng(4040)
    k = (2 * n) // 3
    slab = np.stack([rng.uniform(-1.0, 1.0, k), rng.uniform(-1.0, 1.0, k), rng.uniform(-0.02, 0.02, k)], axis=1)
    slab[:, 2] += 0.3 * slab[:, 0] - 0.2 * slab[:, 1]
    rest = rng.uniform(-1.0, 1.0, (n - k, 3))
    pts = np.concatenate([slab, rest])[rng.permutation(n)]
    return _freeze(np.ascontiguousarray(np.round(pts * 2.0 ** 20) / 2.0 ** 20))


GRID_TAU, GRID_HYP, GRID_SEED = 0.03125, 257, 5


# ------------------------------------------------------------------------------------------------ the restatement's results
@functools.lru_cache(maxsize=None)
def table_result(seed, with_normals=False):
    pts, nrm, _, _ = table_scene()
    if with_normals:
        return op.segment_plane(pts, TAU, N_HYP, seed, 3, nrm, NORMAL_ANGLE)
    return op.segment_plane(pts, TAU, N_HYP, seed)


@functools.lru_cache(maxsize=None)
def room_result():
    pts, _, _ = room_scene()
    return op.segment_planes(pts, TAU, 4, ROOM_MIN_INLIERS, N_HYP, 0)


@functools.lru_cache(maxsize=None)
def grid_result(shifted):
    pts = grid_cloud()
    return op.segment_plane(pts + SHIFT_EXACT if shifted else pts, GRID_TAU, GRID_HYP, GRID_SEED)


def angle_deg(n, m):
    """The angle between two directions (sign ignored), in degrees."""
    c = abs(float(np.dot(n, m))) / (np.linalg.norm(n) * np.linalg.norm(m))
    return float(np.degrees(np.arccos(min(1.0, c))))
