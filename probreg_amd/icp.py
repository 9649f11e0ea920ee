"""ICP, point-to-point and point-to-plane: the polishing step after a global or probabilistic stage, and the baseline the
reference's examples time every method against.

The reference has no counterpart; its examples call Open3D's ``registration_icp`` (``examples/time_measurement.py``,
``examples/icp_test.py``).  Here the nearest-neighbour search on a grid of the target, the ordered sums, the Kabsch /
Cholesky step and Open3D's loop with its stop test all run in ``libprobreg_hip.so`` (``prg_icp_*``, csrc/icp.hip) in fp64.
DESIGN.md section 3.15 is the definition; results are byte-identical from run to run and do not depend on the grid.  Neither
Open3D nor scikit-learn is imported.

    from probreg_amd import global_reg, icp
    start = global_reg.registration_global(source, target, max_distance=0.08)
    res = icp.registration_icp(source, target, 0.05, init=start.transformation)

``evaluate_registration`` scores the result of any method of the library, ``nearest_neighbour`` is the search on its own, and
``IcpPlan`` gives every stage: matches, raw sums, one step, the pose, the loop.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from .engine import _current_device_and_stream
from .global_reg import _as_rows, _single_process
from .transformation import RigidTransformation

POINT_TO_POINT, POINT_TO_PLANE = 0, 1
_KINDS = {"point_to_point": POINT_TO_POINT, "point_to_plane": POINT_TO_PLANE}
STATUS = ("ok", "too_few_matches", "degenerate")
N_SUMS = 32

IcpResult = collections.namedtuple("IcpResult", ["transformation", "fitness", "inlier_rmse", "correspondences", "n_iter",
                                                 "converged"])
IcpState = collections.namedtuple("IcpState", ["pose", "count", "sum", "n_iter", "converged", "status"])


def _check_r(r, name="max_correspondence_distance"):
    r = float(r)
    if not r > 0.0:  # also NaN
        raise ValueError("%s must be > 0 (infinity: no limit), got %r" % (name, r))
    return r


def _kind(estimation):
    if estimation in (POINT_TO_POINT, POINT_TO_PLANE) and not isinstance(estimation, str):
        return int(estimation)
    if estimation not in _KINDS:
        raise ValueError("estimation must be 'point_to_point' or 'point_to_plane', got %r" % (estimation,))
    return _KINDS[estimation]


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


class IcpPlan(object):
    """One ``prg_icp`` handle: a target with its search grid, a source and a pose on one device / stream, and the stages of
    ICP.  ``cell_edge`` overrides the grid's cell edge (it never changes a result)."""

    def __init__(self, device=None):
        _lib.require_gpu()
        dev, st = _current_device_and_stream(device)
        self.device = dev
        self._h = ctypes.c_void_p()
        _lib.check(_lib.lib.prg_icp_create(ctypes.byref(self._h), dev, ctypes.c_void_p(st)))
        self.n_source = 0
        self.n_target = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            _lib.lib.prg_icp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover - interpreter shutdown
            pass

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

    def sums(self, estimation):
        """The raw ordered sums of a step over the current matches (32 doubles, laid out as ``prg_icp_sums`` documents)."""
        out = np.empty(N_SUMS)
        _lib.check(_lib.lib.prg_icp_sums(self._h, _kind(estimation), _lib.ptr(out)))
        return out

    def step(self, estimation):
        """One step on the current matches; a missing step leaves the pose and shows in ``state().status``."""
        _lib.check(_lib.lib.prg_icp_step(self._h, _kind(estimation)))

    def iterate(self, estimation, r, max_iteration=30, relative_fitness=1.0e-6, relative_rmse=1.0e-6, chunk=8):
        _lib.check(_lib.lib.prg_icp_iterate(self._h, _kind(estimation), _check_r(r), int(max_iteration), float(relative_fitness),
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
