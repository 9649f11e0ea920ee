"""ICP, point-to-point and point-to-plane: the polishing step after a global or probabilistic stage, and the baseline the
reference's examples time every method against.

The reference has no counterpart; its examples call Open3D's ``registration_icp`` (``examples/time_measurement.py``,
``examples/icp_test.py``).  Here the nearest-neighbour search on a grid of the target, the ordered sums, the Kabsch /
Cholesky step and Open3D's loop with its stop test all run in ``libprobreg_hip.so`` (``prg_icp_*``, csrc/icp.hip and, for the
search, csrc/grid_search.hip) in fp64.
DESIGN.md section 3.15 is the definition; results are byte-identical from run to run and do not depend on the grid.  Neither
Open3D nor scikit-learn is imported.

    from probreg_amd import global_reg, icp
    start = global_reg.registration_global(source, target, max_distance=0.08)
    res = icp.registration_icp(source, target, 0.05, init=start.transformation)

``evaluate_registration`` scores the result of any method of the library, ``nearest_neighbour`` is the search on its own, and
``IcpPlan`` gives every stage: matches, raw sums, one step, the pose, the loop.

``registration_gicp`` is generalized (plane-to-plane) ICP, Open3D's ``registration_generalized_icp``, on the same search, sums,
step and loop: every point carries a covariance, given or ``I - (1 - epsilon) u u^T`` of its unit normal.

``knn_search`` and ``radius_count`` are the exact k-nearest-neighbour lists (k <= 64) and the radius counts on the same grid
(DESIGN.md section 3.17); ``preprocess.remove_statistical_outlier`` and ``remove_radius_outlier`` are built on them.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from .global_reg import _as_rows, _single_process
from .transformation import RigidTransformation

POINT_TO_POINT, POINT_TO_PLANE = 0, 1
GENERALIZED = 2
PIVOT = 1.0e-12  # a Cholesky pivot <= PIVOT max diag is not positive (the rule of the 6 x 6 step)
_WHICH = {"source": 0, "target": 1}
_KINDS = {"point_to_point": POINT_TO_POINT, "point_to_plane": POINT_TO_PLANE}
STATUS = ("ok", "too_few_matches", "degenerate")
N_SUMS = 32

IcpResult = collections.namedtuple("IcpResult", ["transformation", "fitness", "inlier_rmse", "correspondences", "n_iter",
                                                 "converged"])
IcpState = collections.namedtuple("IcpState", ["pose", "count", "sum", "n_iter", "converged", "status"])
GicpResult = collections.namedtuple("GicpResult", ["transformation", "fitness", "inlier_rmse", "correspondences", "n_iter",
                                                   "converged", "objective"])
KnnResult = collections.namedtuple("KnnResult", ["index", "d2", "count"])
MAX_K = 64  # prg_icp_max_k: one list entry per lane of a wave


def _check_r(r, name="max_correspondence_distance"):
    r = float(r)
    if not r > 0.0:  # also NaN
        raise ValueError("%s must be > 0 (infinity: no limit), got %r" % (name, r))
    return r


def _number(v, name):
    """float(v) of a real number; booleans, strings and whatever float() refuses raise ValueError (NaN passes: the range
    tests of the callers refuse it)."""
    if isinstance(v, (bool, np.bool_, str, bytes)):
        raise ValueError("%s must be a number, got %r" % (name, v))
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (name, v))


def _check_k(k, name="k"):
    """An integer in 1 .. MAX_K (an integral float passes)."""
    v = _number(k, name)
    if not (v == int(v) if np.isfinite(v) else False) or not 1 <= v <= MAX_K:
        raise ValueError("%s must be an integer in 1 .. %d, got %r" % (name, MAX_K, k))
    return int(v)


def _check_radius(r, name, allow_inf):
    v = _number(r, name)
    if not v > 0.0 or (not allow_inf and not np.isfinite(v)):  # also NaN
        raise ValueError("%s must be %s> 0%s, got %r" % (name, "" if allow_inf else "finite and ",
                                                       " (infinity: no limit)" if allow_inf else "", r))
    return v


def _kind(estimation):
    if estimation in (POINT_TO_POINT, POINT_TO_PLANE) and not isinstance(estimation, str):
        return int(estimation)
    if estimation not in _KINDS:
        raise ValueError("estimation must be 'point_to_point' or 'point_to_plane', got %r" % (estimation,))
    return _KINDS[estimation]


def _plan_kind(estimation):
    """``_kind`` and, for the stages of a plan, the generalized estimator."""
    if (estimation == GENERALIZED and not isinstance(estimation, str)) or estimation == "generalized":
        return GENERALIZED
    return _kind(estimation)


def _check_epsilon(epsilon):
    eps = float(epsilon)
    if not 0.0 < eps <= 1.0:  # also NaN
        raise ValueError("epsilon must lie in (0, 1], got %r" % (epsilon,))
    return eps


def _checked_normals(normals, name, n=None):
    """(normals (n, 3), their lengths): finite, one row per point, no length 0."""
    nrm = _as_rows(normals, name, 3)
    if n is not None and nrm.shape[0] != n:
        raise ValueError("%s must have one row per point (%d), got %d" % (name, n, nrm.shape[0]))
    with np.errstate(over="ignore"):
        length = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
    bad = np.nonzero(~(np.isfinite(length) & (length > 0.0)))[0]
    if bad.size:
        raise ValueError("%s: row %d has norm 0 (or one that is not finite); a covariance needs a direction"
                         % (name, int(bad[0])))
    return nrm, length


def _cov6_from_normals(nrm, length, eps):
    """The host mirror of the device's covariances from normals, (n, 6): xx, xy, xz, yy, yz, zz."""
    u = nrm / length[:, None]
    w = (1.0 - eps) * u
    c = np.empty((nrm.shape[0], 6))
    c[:, 0] = 1.0 - w[:, 0] * u[:, 0]
    c[:, 1] = -(w[:, 0] * u[:, 1])
    c[:, 2] = -(w[:, 0] * u[:, 2])
    c[:, 3] = 1.0 - w[:, 1] * u[:, 1]
    c[:, 4] = -(w[:, 1] * u[:, 2])
    c[:, 5] = 1.0 - w[:, 2] * u[:, 2]
    return c


def _full(c6):
    return np.ascontiguousarray(c6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3))


def covariances_from_normals(normals, epsilon=1.0e-3):
    """(n, 3, 3): ``C = I - (1 - epsilon) u u^T`` of the unit normals ``u = n / |n|`` - Open3D's ``R diag(epsilon, 1, 1) R^T``,
    whatever the sign of the normal.  The host mirror of what ``set_source_covariances(normals=...)`` computes on the
    device, operation for operation."""
    eps = _check_epsilon(epsilon)
    nrm, length = _checked_normals(normals, "normals")
    return _full(_cov6_from_normals(nrm, length, eps))


def _checked_cov6(covariances, name, n=None):
    """(n, 6) of covariances given as (n, 3, 3) or (n, 6): finite, symmetric, positive definite by the pivot rule."""
    c = np.asarray(covariances, dtype=np.float64)
    if c.ndim == 3 and c.shape[0] >= 1 and c.shape[1:] == (3, 3):
        if not np.all(np.isfinite(c)):
            raise ValueError("%s contains NaN or infinity" % name)
        if not np.array_equal(c, c.transpose(0, 2, 1)):
            raise ValueError("%s must be symmetric" % name)
        c = c.reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]]
    elif c.ndim == 2 and c.shape[0] >= 1 and c.shape[1] == 6:
        if not np.all(np.isfinite(c)):
            raise ValueError("%s contains NaN or infinity" % name)
    else:
        raise ValueError("%s must be (n, 3, 3) or (n, 6: xx, xy, xz, yy, yz, zz) with n >= 1, got shape %s" % (name, c.shape))
    if n is not None and c.shape[0] != n:
        raise ValueError("%s must have one covariance per point (%d), got %d" % (name, n, c.shape[0]))
    c = np.ascontiguousarray(c)
    floor = PIVOT * np.max(c[:, [0, 3, 5]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        l00 = np.sqrt(c[:, 0])
        l10, l20 = c[:, 1] / l00, c[:, 2] / l00
        d1 = c[:, 3] - l10 * l10
        l11 = np.sqrt(d1)
        l21 = (c[:, 4] - l20 * l10) / l11
        d2 = (c[:, 5] - l20 * l20) - l21 * l21
        good = (c[:, 0] > floor) & (d1 > floor) & (d2 > floor)
    bad = np.nonzero(~good)[0]
    if bad.size:
        raise ValueError("%s: covariance %d is not positive definite (a Cholesky pivot <= 1e-12 max diag)" % (name, int(bad[0])))
    return c


def _pose12(init):
    """12 doubles (rotation row-major, then the shift) of None, a RigidTransformation with scale 1 or a 4 x 4 array."""
    if init is None:
        return np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    if hasattr(init, "rot") and hasattr(init, "t"):
        if float(getattr(init, "scale", 1.0)) != 1.0:
            raise ValueError("init must have scale 1 (ICP estimates no scale), got %r" % (init.scale,))
        rot, t = np.asarray(init.rot, dtype=np.float64), np.asarray(init.t, dtype=np.float64)
    else:
        m = np.asarray(init, dtype=np.float64)
        if m.shape != (4, 4):
            raise ValueError("init must be None, a RigidTransformation or a 4 x 4 array, got shape %s" % (m.shape,))
        if not np.array_equal(m[3], [0.0, 0.0, 0.0, 1.0]):
            raise ValueError("the last row of init must be (0, 0, 0, 1)")
        rot, t = m[:3, :3], m[:3, 3]
    if rot.shape != (3, 3) or t.shape != (3,):
        raise ValueError("init must hold a 3 x 3 rotation and a shift of 3, got %s and %s" % (rot.shape, t.shape))
    pose = np.concatenate([rot.reshape(9), t])
    if not np.all(np.isfinite(pose)):
        raise ValueError("init contains NaN or infinity")
    return np.ascontiguousarray(pose)


def _normals_of(target, target_normals, n):
    nrm = target_normals if target_normals is not None else getattr(target, "normals", None)
    if nrm is None or (hasattr(nrm, "__len__") and len(nrm) == 0):
        raise ValueError("point-to-plane ICP needs the target's normals: pass target_normals (n, 3) or a target with "
                         ".normals; fpfh.FPFH().estimate_normals(target) computes them")
    nrm = _as_rows(nrm, "target_normals", 3)
    if nrm.shape[0] != n:
        raise ValueError("target_normals must have one row per target point (%d), got %d" % (n, nrm.shape[0]))
    return nrm


class IcpPlan(_lib.Handle):
    """One ``prg_icp`` handle: a target with its search grid, a source and a pose on one device / stream, and the stages of
    ICP.  ``cell_edge`` overrides the grid's cell edge (it never changes a result)."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_icp_create, _lib.lib.prg_icp_destroy, device)
        self.n_source = 0
        self.n_target = 0

    def set_target(self, points, normals=None, cell_edge=None):
        pts = _as_rows(points, "target", 3)
        nrm = None
        if normals is not None:
            nrm = _as_rows(normals, "target_normals", 3)
            if nrm.shape != pts.shape:
                raise ValueError("target_normals must have the shape of target %s, got %s" % (pts.shape, nrm.shape))
        edge = 0.0
        if cell_edge is not None:
            edge = float(cell_edge)
            if not (np.isfinite(edge) and edge > 0.0):
                raise ValueError("cell_edge must be finite and > 0, got %r" % (cell_edge,))
        _lib.check(_lib.lib.prg_icp_set_target(self._h, _lib.ptr(pts), _lib.ptr(nrm), pts.shape[0], edge))
        self.n_target = pts.shape[0]

    def grid(self):
        """(cell edge of the finest level, its cells per axis (3,), dense: True when its cells are addressed directly and
        False when hashed, number of levels)."""
        edge, dense, levels = ctypes.c_double(0.0), ctypes.c_int(0), ctypes.c_int(0)
        dims = np.zeros(3, dtype=np.int32)
        _lib.check(_lib.lib.prg_icp_get_grid(self._h, ctypes.byref(edge), _lib.ptr(dims), ctypes.byref(dense),
                                             ctypes.byref(levels)))
        return float(edge.value), dims, bool(dense.value), int(levels.value)

    def set_source(self, points):
        pts = _as_rows(points, "source", 3)
        _lib.check(_lib.lib.prg_icp_set_source(self._h, _lib.ptr(pts), pts.shape[0]))
        self.n_source = pts.shape[0]

    def _set_covariances(self, which, n, covariances, normals, epsilon):
        name = "%s_covariances" % which
        if (covariances is None) == (normals is None):
            raise ValueError("set_%s takes either covariances or normals" % name)
        if n < 1:
            raise ValueError("set_%s: set the %s first (its covariances go with it)" % (name, which))
        if covariances is not None:
            c = _checked_cov6(covariances, name, n)
            _lib.check(_lib.lib.prg_icp_set_covariances(self._h, _WHICH[which], _lib.ptr(c), n))
        else:
            eps = _check_epsilon(epsilon)
            nrm, _ = _checked_normals(normals, "%s_normals" % which, n)
            _lib.check(_lib.lib.prg_icp_set_covariances_from_normals(self._h, _WHICH[which], _lib.ptr(nrm), n, eps))

    def set_source_covariances(self, covariances=None, normals=None, epsilon=1.0e-3):
        """The source's covariances for the generalized estimator: ``covariances`` (M, 3, 3) or (M, 6: xx, xy, xz, yy, yz, zz),
        symmetric positive definite, or ``normals`` (M, 3) with ``epsilon`` (``covariances_from_normals``, on the device).
        After ``set_source``, which drops them."""
        self._set_covariances("source", self.n_source, covariances, normals, epsilon)

    def set_target_covariances(self, covariances=None, normals=None, epsilon=1.0e-3):
        """The target's covariances, as ``set_source_covariances``.  After ``set_target``, which drops them."""
        self._set_covariances("target", self.n_target, covariances, normals, epsilon)

    def covariances(self, which):
        """(n, 3, 3): the covariances of ``which`` ("source" or "target") as the device holds them."""
        if which not in _WHICH:
            raise ValueError("which must be 'source' or 'target', got %r" % (which,))
        c = np.empty((self.n_source if which == "source" else self.n_target, 6))
        _lib.check(_lib.lib.prg_icp_get_covariances(self._h, _WHICH[which], _lib.ptr(c)))
        return _full(c)

    def set_pose(self, pose):
        """``pose``: None, a RigidTransformation with scale 1, a 4 x 4 array or 12 doubles (rotation row-major, then the shift)."""
        p = np.asarray(pose, dtype=np.float64) if pose is not None and not hasattr(pose, "rot") else None
        if p is not None and p.shape == (12,):
            if not np.all(np.isfinite(p)):
                raise ValueError("pose contains NaN or infinity")
            p = np.ascontiguousarray(p)
        else:
            p = _pose12(pose)
        _lib.check(_lib.lib.prg_icp_set_pose(self._h, _lib.ptr(p)))

    def pose(self):
        p = np.empty(12)
        _lib.check(_lib.lib.prg_icp_get_pose(self._h, _lib.ptr(p)))
        return p

    def search(self, r):
        _lib.check(_lib.lib.prg_icp_search(self._h, _check_r(r)))

    def matches(self):
        """(index (M,) int32 with -1 where nothing lies within r, d2 (M,) with +inf there)."""
        idx = np.empty(self.n_source, dtype=np.int32)
        d2 = np.empty(self.n_source)
        _lib.check(_lib.lib.prg_icp_get_matches(self._h, _lib.ptr(idx), _lib.ptr(d2)))
        return idx, d2

    def knn(self, k, r=np.inf):
        """``KnnResult(index (M, k) int32, d2 (M, k), count (M,) int32)``: for every moved source point the targets with
        ``d2 <= r r`` in ascending ``(d2, index)``, cut to ``k`` (1 .. 64) entries; the slots past ``count`` hold -1 and
        +inf.  ``k = 1`` is ``search`` + ``matches``."""
        k, r = _check_k(k), _check_radius(r, "r", True)
        _lib.check(_lib.lib.prg_icp_knn(self._h, k, r))
        return self._lists(k)

    def _lists(self, k):
        idx = np.empty((self.n_source, k), dtype=np.int32)
        d2 = np.empty((self.n_source, k))
        cnt = np.empty(self.n_source, dtype=np.int32)
        _lib.check(_lib.lib.prg_icp_get_knn(self._h, _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt)))
        return KnnResult(idx, d2, cnt)

    def radius_count(self, r):
        """(M,) int32: for every moved source point the number of targets with ``d2 <= r r``; ``r`` finite."""
        _lib.check(_lib.lib.prg_icp_radius_count(self._h, _check_radius(r, "r", False)))
        return self._counts()

    def _counts(self):
        cnt = np.empty(self.n_source, dtype=np.int32)
        _lib.check(_lib.lib.prg_icp_get_counts(self._h, _lib.ptr(cnt)))
        return cnt

    def _outlier_statistical(self, k, std_ratio):
        """For ``preprocess.remove_statistical_outlier``, which has checked the arguments and set one cloud as source and as
        target at the identity pose: (keep (M,) bool, a (M,), (mu, s, thr))."""
        _lib.check(_lib.lib.prg_icp_outlier_statistical(self._h, k, std_ratio))
        keep = np.empty(self.n_source, dtype=np.uint8)
        score, stat = np.empty(self.n_source), np.empty(3)
        _lib.check(_lib.lib.prg_icp_get_outlier(self._h, _lib.ptr(keep), _lib.ptr(score), _lib.ptr(stat)))
        return keep.astype(bool), score, (float(stat[0]), float(stat[1]), float(stat[2]))

    def _outlier_radius(self, nb_points, radius):
        """For ``preprocess.remove_radius_outlier``, as ``_outlier_statistical``: (keep (M,) bool, counts (M,) int32)."""
        _lib.check(_lib.lib.prg_icp_outlier_radius(self._h, radius, nb_points))
        keep = np.empty(self.n_source, dtype=np.uint8)
        _lib.check(_lib.lib.prg_icp_get_outlier(self._h, _lib.ptr(keep), None, None))
        return keep.astype(bool), self._counts()

    def _dbscan(self, eps, min_points):
        """For ``preprocess.cluster_dbscan``, as ``_outlier_statistical``: (labels (M,) int32, core (M,) bool, counts (M,) int32,
        n_clusters, sizes (n_clusters,) int32)."""
        _lib.check(_lib.lib.prg_icp_dbscan(self._h, eps, min_points))
        labels = np.empty(self.n_source, dtype=np.int32)
        core = np.empty(self.n_source, dtype=np.uint8)
        n_clusters = ctypes.c_int(0)
        _lib.check(_lib.lib.prg_icp_get_dbscan(self._h, _lib.ptr(labels), _lib.ptr(core), ctypes.byref(n_clusters), None))
        sizes = np.empty(int(n_clusters.value), dtype=np.int32)
        if sizes.shape[0] > 0:
            _lib.check(_lib.lib.prg_icp_get_dbscan(self._h, None, None, None, _lib.ptr(sizes)))
        return labels, core.astype(bool), self._counts(), int(n_clusters.value), sizes

    def sums(self, estimation):
        """The raw ordered sums of a step over the current matches (32 doubles, laid out as ``prg_icp_sums`` documents).
        ``estimation``: as in ``registration_icp``, or ``GENERALIZED`` / "generalized" (here, in ``step`` and in ``iterate``)."""
        out = np.empty(N_SUMS)
        _lib.check(_lib.lib.prg_icp_sums(self._h, _plan_kind(estimation), _lib.ptr(out)))
        return out

    def step(self, estimation):
        """One step on the current matches; a missing step leaves the pose and shows in ``state().status``."""
        _lib.check(_lib.lib.prg_icp_step(self._h, _plan_kind(estimation)))

    def iterate(self, estimation, r, max_iteration=30, relative_fitness=1.0e-6, relative_rmse=1.0e-6, chunk=8):
        _lib.check(_lib.lib.prg_icp_iterate(self._h, _plan_kind(estimation), _check_r(r), int(max_iteration), float(relative_fitness),
                                            float(relative_rmse), int(chunk)))

    def state(self):
        """IcpState(pose (12,), count, sum, n_iter, converged, status) of the last evaluation / loop."""
        pose = np.empty(12)
        cnt, sm = ctypes.c_int64(0), ctypes.c_double(0.0)
        it, conv, status = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(_lib.lib.prg_icp_get_state(self._h, _lib.ptr(pose), ctypes.byref(cnt), ctypes.byref(sm), ctypes.byref(it),
                                              ctypes.byref(conv), ctypes.byref(status)))
        return IcpState(pose, int(cnt.value), float(sm.value), int(it.value), bool(conv.value), STATUS[status.value])


def _correspondences(idx):
    src = np.nonzero(idx >= 0)[0].astype(np.int32)
    return np.stack([src, idx[src]], axis=1).astype(np.int32)


def _score(count, total, m):
    return count / float(m), float(np.sqrt(total / count)) if count else 0.0


def _check_loop(max_iteration, relative_fitness, relative_rmse):
    if int(max_iteration) != max_iteration or max_iteration < 0:
        raise ValueError("max_iteration must be an integer >= 0, got %r" % (max_iteration,))
    if not (np.isfinite(relative_fitness) and np.isfinite(relative_rmse)):
        raise ValueError("relative_fitness and relative_rmse must be finite")


def registration_icp(source, target, max_correspondence_distance, init=None, estimation="point_to_point", target_normals=None,
                     max_iteration=30, relative_fitness=1.0e-6, relative_rmse=1.0e-6, device=None):
    """Open3D's ``registration_icp``: from the pose ``init`` (None, a ``RigidTransformation`` with scale 1 such as
    ``GlobalResult.transformation``, or a 4 x 4 array), match every moved source point to its nearest target point within
    ``max_correspondence_distance`` (``inf``: no limit), take a point-to-point (Kabsch) or point-to-plane step, and repeat
    until fitness and inlier_rmse both change by less than the two thresholds or ``max_iteration`` steps are done.

    ``IcpResult(transformation, fitness, inlier_rmse, correspondences, n_iter, converged)``: ``transformation`` is a
    ``RigidTransformation`` with scale 1; ``fitness`` = matched / len(source), ``inlier_rmse`` over the matches and
    ``correspondences`` (K, 2) int32 of (source, target) indices, all at the final pose; ``n_iter`` counts the steps done.
    A step that cannot be taken (fewer than 3 matches; point-to-plane: fewer than 6 or a degenerate system) ends the loop
    with the pose as it is and ``converged`` False.  Point-to-plane takes ``target_normals`` or ``target.normals``."""
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    r = _check_r(max_correspondence_distance)
    kind = _kind(estimation)
    pose = _pose12(init)
    nrm = _normals_of(target, target_normals, tgt.shape[0]) if kind == POINT_TO_PLANE else None
    _check_loop(max_iteration, relative_fitness, relative_rmse)
    _single_process("registration_icp")
    plan = IcpPlan(device)
    try:
        plan.set_target(tgt, nrm)
        plan.set_source(src)
        plan.set_pose(pose)
        plan.iterate(kind, r, max_iteration, relative_fitness, relative_rmse)
        st = plan.state()
        idx, _ = plan.matches()
    finally:
        plan.close()
    fitness, rmse = _score(st.count, st.sum, src.shape[0])
    tf = RigidTransformation(st.pose[:9].reshape(3, 3).copy(), st.pose[9:].copy(), 1.0)
    return IcpResult(tf, fitness, rmse, _correspondences(idx), st.n_iter, st.converged)


def _gicp_covariances(cloud, name, n, covariances, normals, normal_radius):
    """What ``registration_gicp`` hands to the plan for one cloud: ("covariances", (n, 6)), ("normals", (n, 3)) or
    ("estimate", None), from the first source that applies; everything given is validated here, on the host."""
    if covariances is not None:
        return "covariances", _checked_cov6(covariances, "%s_covariances" % name, n)
    nrm = normals if normals is not None else getattr(cloud, "normals", None)
    if nrm is not None and not (hasattr(nrm, "__len__") and len(nrm) == 0):
        return "normals", _checked_normals(nrm, "%s_normals" % name, n)[0]
    if normal_radius is None:
        raise ValueError("generalized ICP needs covariances or normals of the %s: pass %s_covariances, %s_normals, a %s with "
                         ".normals, or normal_radius (then fpfh.FPFH(radius_normal=normal_radius).estimate_normals computes "
                         "them)" % (name, name, name, name))
    return "estimate", None


def registration_gicp(source, target, max_correspondence_distance, init=None, source_normals=None, target_normals=None,
                      source_covariances=None, target_covariances=None, epsilon=1.0e-3, normal_radius=None, normal_max_nn=30,
                      max_iteration=30, relative_fitness=1.0e-6, relative_rmse=1.0e-6, device=None):
    """Generalized (plane-to-plane) ICP, Open3D's ``registration_generalized_icp``: the loop, the search and the stop test
    of ``registration_icp``; a step minimises ``sum d^T (C_target + R C_source R^T)^-1 d`` over the matches, linearised at
    the current pose.

    A cloud gets its covariances from the first of: its ``*_covariances`` argument ((n, 3, 3) or (n, 6), symmetric positive
    definite); its ``*_normals`` argument; its ``.normals`` attribute; ``fpfh.FPFH(radius_normal=normal_radius,
    max_nn_normal=normal_max_nn).estimate_normals`` when ``normal_radius`` is given.  Normals become
    ``I - (1 - epsilon) u u^T``, ``0 < epsilon <= 1``.

    ``GicpResult(transformation, fitness, inlier_rmse, correspondences, n_iter, converged, objective)``: as ``IcpResult``
    (fitness and inlier_rmse are Euclidean), and ``objective`` the Mahalanobis sum over the final matches at the final pose.
    A step that cannot be taken (fewer than 6 matches, a degenerate system) ends the loop with ``converged`` False."""
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    r = _check_r(max_correspondence_distance)
    pose = _pose12(init)
    eps = _check_epsilon(epsilon)
    if normal_radius is not None and not (np.isfinite(normal_radius) and normal_radius > 0.0):
        raise ValueError("normal_radius must be > 0 and finite, got %r" % (normal_radius,))
    how = [_gicp_covariances(source, "source", src.shape[0], source_covariances, source_normals, normal_radius),
           _gicp_covariances(target, "target", tgt.shape[0], target_covariances, target_normals, normal_radius)]
    _check_loop(max_iteration, relative_fitness, relative_rmse)
    _single_process("registration_gicp")
    for k, pts in enumerate((src, tgt)):
        if how[k][0] == "estimate":
            from . import fpfh

            est = fpfh.FPFH(radius_normal=normal_radius, max_nn_normal=normal_max_nn, device=device).estimate_normals(pts)
            how[k] = ("normals", _checked_normals(est, "the estimated %s normals" % ("source", "target")[k], pts.shape[0])[0])
    plan = IcpPlan(device)
    try:
        plan.set_target(tgt)
        plan.set_source(src)
        for setter, (what, value) in zip((plan.set_source_covariances, plan.set_target_covariances), how):
            setter(**{what: value, "epsilon": eps})
        plan.set_pose(pose)
        plan.iterate(GENERALIZED, r, max_iteration, relative_fitness, relative_rmse)
        st = plan.state()
        idx, _ = plan.matches()
        objective = float(plan.sums(GENERALIZED)[29])
    finally:
        plan.close()
    fitness, rmse = _score(st.count, st.sum, src.shape[0])
    tf = RigidTransformation(st.pose[:9].reshape(3, 3).copy(), st.pose[9:].copy(), 1.0)
    return GicpResult(tf, fitness, rmse, _correspondences(idx), st.n_iter, st.converged, objective)


def evaluate_registration(source, target, max_correspondence_distance, transformation=None, device=None):
    """Open3D's ``evaluate_registration``: ``(fitness, inlier_rmse, correspondences)`` of ``transformation``: None, a 4 x 4
    array, or the result of any method of the library.  A ``RigidTransformation`` with scale 1 moves the source on the device
    by the definition's own formula; anything else with ``.transform`` (a scaled rigid, affine, non-rigid, thin-plate-spline
    or combined transformation) is applied to the source on the host first and the moved cloud is scored at the identity."""
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    r = _check_r(max_correspondence_distance)
    rigid = hasattr(transformation, "rot") and hasattr(transformation, "t") and float(getattr(transformation, "scale", 1.0)) == 1.0
    if transformation is not None and not rigid and callable(getattr(transformation, "transform", None)):
        moved = _as_rows(transformation.transform(src), "transformation.transform(source)", 3)
        if moved.shape != src.shape:
            raise ValueError("transformation.transform(source) must keep the shape %s, got %s" % (src.shape, moved.shape))
        src, transformation = moved, None
    pose = _pose12(transformation)
    _single_process("evaluate_registration")
    plan = IcpPlan(device)
    try:
        plan.set_target(tgt)
        plan.set_source(src)
        plan.set_pose(pose)
        plan.iterate(POINT_TO_POINT, r, 0)
        st = plan.state()
        idx, _ = plan.matches()
    finally:
        plan.close()
    fitness, rmse = _score(st.count, st.sum, src.shape[0])
    return fitness, rmse, _correspondences(idx)


def nearest_neighbour(query, cloud, max_distance=None, device=None):
    """(index (M,) int32, d2 (M,)): for every row of ``query`` the row of ``cloud`` of least squared distance
    ``(dx dx + dy dy) + dz dz``, ties to the smaller index; with ``max_distance`` rows farther than that get (-1, inf).
    Exact at any size: the grid search looks at what a brute-force sweep would find."""
    q, c = _as_rows(query, "query", 3), _as_rows(cloud, "cloud", 3)
    r = np.inf if max_distance is None else _check_r(max_distance, "max_distance")
    _single_process("nearest_neighbour")
    plan = IcpPlan(device)
    try:
        plan.set_target(c)
        plan.set_source(q)
        plan.search(r)
        return plan.matches()
    finally:
        plan.close()


def knn_search(query, cloud, k, max_distance=None, device=None):
    """``KnnResult(index (Q, k) int32, d2 (Q, k), count (Q,) int32)``: for every row of ``query`` the ``k`` (1 .. 64) rows of
    ``cloud`` of least squared distance ``(dx dx + dy dy) + dz dz``, ascending, ties to the smaller index; with
    ``max_distance`` only rows within it (``d2 <= r r``) are listed.  Slots past ``count`` hold -1 and +inf.  Exact at any
    size.  When ``query`` is ``cloud`` a point is an ordinary candidate at ``d2 = 0``: it comes
    first unless a copy of it has a smaller index."""
    q, c = _as_rows(query, "query", 3), _as_rows(cloud, "cloud", 3)
    k = _check_k(k)
    r = np.inf if max_distance is None else _check_radius(max_distance, "max_distance", True)
    _single_process("knn_search")
    plan = IcpPlan(device)
    try:
        plan.set_target(c)
        plan.set_source(q)
        return plan.knn(k, r)
    finally:
        plan.close()


def radius_count(query, cloud, radius, device=None):
    """(Q,) int32: for every row of ``query`` the number of rows of ``cloud`` with ``d2 <= radius radius``."""
    q, c = _as_rows(query, "query", 3), _as_rows(cloud, "cloud", 3)
    r = _check_radius(radius, "radius", False)
    _single_process("radius_count")
    plan = IcpPlan(device)
    try:
        plan.set_target(c)
        plan.set_source(q)
        return plan.radius_count(r)
    finally:
        plan.close()
