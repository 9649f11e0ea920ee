"""Preprocessing of clouds: ``voxel_down_sample``, the first step of every 3-D example of the reference.

The reference has no counterpart; its examples call Open3D's ``voxel_down_sample(voxel_size)`` on both clouds before they
register (examples/utils.py: ``prepare_source_and_target_rigid_3d``, ``prepare_source_and_target_nonrigid_3d``).  Here it
runs in ``libprobreg_hip.so`` (``prg_voxel_*``, csrc/voxel.hip) in fp64: a 64-bit cell key per point, a stable device radix
sort and a segmented sum in a fixed order.  DESIGN.md section 3.14 is the definition; results are byte-identical from run
to run.  Neither Open3D nor scikit-learn is imported.

Differences from Open3D a caller can see (on purpose):
  * The output voxels come in ascending cell order (x, then y, then z); Open3D's order is that of its hash map.
  * An axis may span at most 2^21 cells (Open3D: INT_MAX); a larger grid raises ``ValueError``.
  * Arrays go in and come out: ``VoxelDownSample(points, normals, attributes, counts, first, inverse)``.

``remove_statistical_outlier`` and ``remove_radius_outlier`` are Open3D's filters of those names, which clean a cloud of the
uniform outliers the reference's example set-up adds to every target (examples/utils.py: ``n_random``).  They run on the exact
k-nearest-neighbour search and the radius count of ``probreg_amd.icp`` (``prg_icp_knn``, ``prg_icp_radius_count``, csrc/grid_search.hip; the filters: csrc/icp_outlier.hip;
DESIGN.md section 3.17), in fp64 with every sum in a stated order.

``cluster_dbscan`` is Open3D's ``cluster_dbscan(eps, min_points)``, which cuts a scene into its objects and marks the stray
points between them as noise; ``DbscanResult.clusters()`` hands the objects to ``cpd.registration_cpd_batch``.  It runs on
the same radius count and the same walk of the grid (``prg_icp_dbscan``, csrc/icp_cluster.hip): core
points from the counts, their connected components by a union-find that only ever lowers 32-bit indices with integer
atomics (csrc/union_find.h), clusters numbered by their smallest core index.  Core points, their labels and the noise are
scikit-learn's; a border point goes to the cluster of its nearest core neighbour, not to the one a scan reaches first.

``segment_plane`` is Open3D's ``segment_plane(distance_threshold, ransac_n=3, num_iterations)``, which takes the table or
floor out of a scene before ``cluster_dbscan`` (otherwise the supporting plane is the largest "cluster" and joins everything
that stands on it); ``segment_planes`` repeats it on what is left.  It runs in ``prg_plane_*`` (csrc/plane_seg.hip; the
decisions in the host-compilable csrc/plane_seg.h) in fp64 with every operation rounded once:
counter-based draws, a sweep hypotheses x points with ordered sums, the winner by (count, sum, index), least-squares refits::

    seg = preprocess.segment_plane(scene, 0.01)
    rest = scene[~seg.mask]
    objects = preprocess.cluster_dbscan(rest, eps, min_points).clusters(min_size)
    results = cpd.registration_cpd_batch([model] * len(objects), [rest[i] for i in objects], "rigid")

The result of a global registration on the down-sampled clouds starts a local one on the full clouds::

    from probreg_amd import cpd, global_reg
    res = global_reg.registration_global(source, target, max_distance=0.08, voxel_size=0.05)
    tf = cpd.registration_cpd(source, target, tf_init_params=dict(rot=res.transformation.rot, t=res.transformation.t))
"""
import collections
import ctypes

import numpy as np

from . import _lib
from . import dist as pdist

MAX_ATTRIBUTES = 64
MAX_CELLS = 1 << 21

VoxelDownSample = collections.namedtuple("VoxelDownSample", ["points", "normals", "attributes", "counts", "first", "inverse"])


def _as_channel(a, name, n, cols, max_cols=None):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != n:
        raise ValueError("%s must have one row per point (%d), got shape %s" % (name, n, a.shape))
    if cols is not None and a.shape[1] != cols:
        raise ValueError("%s must be (%d, %d), got shape %s" % (name, n, cols, a.shape))
    if max_cols is not None and not 1 <= a.shape[1] <= max_cols:
        raise ValueError("%s must have 1 .. %d columns, got %d" % (name, max_cols, a.shape[1]))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s contains NaN or infinity" % name)
    return a


def _check_voxel_size(v):
    try:
        size = float("nan") if isinstance(v, (bool, str, bytes)) else float(v)
    except (TypeError, ValueError):
        size = float("nan")
    if not (np.isfinite(size) and size > 0.0):
        raise ValueError("voxel_size must be a finite number > 0, got %r" % (v,))
    return size


def _single_process(what):
    if pdist.world()[1] > 1:
        raise NotImplementedError("%s: sharding over %d ranks is not supported; run it in one process."
                                  % (what, pdist.world()[1]))


class VoxelPlan(_lib.Handle):
    """One ``prg_voxel`` handle: a cloud on one device / stream and the stages of the down-sampling.  A plan can be run
    again with other data or another voxel size."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_voxel_create, _lib.lib.prg_voxel_destroy, device)
        self.n = 0
        self.dim = 0
        self.n_channels = 0

    def set_data(self, points):
        """The cloud (n, 2) or (n, 3); the channels of an earlier cloud go."""
        points = _lib.as_cloud(points, "points", (2, 3))
        _lib.check(_lib.lib.prg_voxel_set_data(self._h, _lib.ptr(points), points.shape[0], points.shape[1]))
        self.n, self.dim = points.shape
        self.n_channels = 0

    def set_channels(self, channels):
        """Per-point channels (n, c) that are averaged like the coordinates; ``None`` removes them."""
        if channels is None:
            _lib.check(_lib.lib.prg_voxel_set_channels(self._h, None, 0))
            self.n_channels = 0
            return
        channels = _as_channel(channels, "channels", self.n, None, MAX_ATTRIBUTES + 3)
        _lib.check(_lib.lib.prg_voxel_set_channels(self._h, _lib.ptr(channels), channels.shape[1]))
        self.n_channels = channels.shape[1]

    def run(self, voxel_size):
        _lib.check(_lib.lib.prg_voxel_run(self._h, _check_voxel_size(voxel_size)))

    def count(self):
        """The number of voxels V."""
        v = ctypes.c_int64(0)
        _lib.check(_lib.lib.prg_voxel_count(self._h, ctypes.byref(v)))
        return int(v.value)

    def _get(self, fn, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        _lib.check(fn(self._h, _lib.ptr(out)))
        return out

    def keys(self):
        """The cell key ``c_x 2^42 + c_y 2^21 + c_z`` of every point, (n,) uint64."""
        self.count()
        return self._get(_lib.lib.prg_voxel_get_keys, self.n, np.uint64)

    def order(self):
        """The point at every position of the sequence stably sorted by key, (n,) int32."""
        self.count()
        return self._get(_lib.lib.prg_voxel_get_order, self.n, np.int32)

    def rows(self):
        """The voxel row of every sorted position, (n,) int32."""
        self.count()
        return self._get(_lib.lib.prg_voxel_get_rows, self.n, np.int32)

    def means(self):
        """The mean point of every voxel, (V, d)."""
        return self._get(_lib.lib.prg_voxel_get_means, (self.count(), self.dim), np.float64)

    def channel_means(self):
        """The mean channels of every voxel, (V, c)."""
        return self._get(_lib.lib.prg_voxel_get_channel_means, (self.count(), self.n_channels), np.float64)

    def counts(self):
        return self._get(_lib.lib.prg_voxel_get_counts, self.count(), np.int32)

    def first(self):
        """The smallest original index in every voxel, (V,) int32."""
        return self._get(_lib.lib.prg_voxel_get_first, self.count(), np.int32)

    def inverse(self):
        """The voxel row of every input point, (n,) int32."""
        self.count()
        return self._get(_lib.lib.prg_voxel_get_inverse, self.n, np.int32)


def _unit_rows(a):
    """Rows divided by their Euclidean norm (squares summed over the columns in ascending order); rows of norm 0 stay 0."""
    sq = np.zeros(a.shape[0])
    for k in range(a.shape[1]):
        sq = sq + a[:, k] * a[:, k]
    norm = np.sqrt(sq)
    return a / np.where(norm > 0.0, norm, 1.0)[:, None]


def voxel_down_sample(points, voxel_size, normals=None, attributes=None, unit_normals=False, device=None):
    """One point per occupied cell of a grid of pitch ``voxel_size``: the mean of the cell's points (Open3D's
    ``voxel_down_sample``).

    Args:
        points: (n, 2) or (n, 3) array, or anything with ``.points``.  An object's ``.normals`` is used when ``normals`` is
            None and it has as many rows as the cloud.
        voxel_size: pitch of the grid, > 0.  The grid starts at ``min - voxel_size / 2`` per axis, as Open3D's.
        normals: (n, d), averaged like the points; the means are not renormalised (as in Open3D) unless ``unit_normals``.
        attributes: (n, c) with 1 <= c <= 64 (colours, intensities, ...), averaged like the points.
        unit_normals: divide every mean normal by its Euclidean norm (on the host); a mean of norm 0 stays 0.
    Returns:
        ``VoxelDownSample(points (V, d), normals (V, d) or None, attributes (V, c) or None, counts (V,) int32,
        first (V,) int32: the smallest original index in the voxel, inverse (n,) int32: the voxel row of every input
        point)``.  Voxels are in ascending cell order (x, then y, then z).
    """
    pts = _lib.as_cloud(points, "points", (2, 3))
    n, d = pts.shape
    v = _check_voxel_size(voxel_size)
    if normals is None and not isinstance(points, np.ndarray) and hasattr(points, "points"):
        own = getattr(points, "normals", None)
        if own is not None and np.ndim(own) == 2 and np.shape(own)[0] == n:
            normals = own
    if normals is not None:
        normals = _as_channel(normals, "normals", n, d)
    if attributes is not None:
        attributes = _as_channel(attributes, "attributes", n, None, MAX_ATTRIBUTES)
    _single_process("voxel_down_sample")
    channels = [a for a in (normals, attributes) if a is not None]
    plan = VoxelPlan(device)
    try:
        plan.set_data(pts)
        if channels:
            plan.set_channels(np.concatenate(channels, axis=1))
        plan.run(v)
        means, counts, first, inverse = plan.means(), plan.counts(), plan.first(), plan.inverse()
        cm = plan.channel_means() if channels else None
    finally:
        plan.close()
    out_normals = out_attributes = None
    if normals is not None:
        out_normals = np.ascontiguousarray(cm[:, :d])
        if unit_normals:
            out_normals = _unit_rows(out_normals)
    if attributes is not None:
        out_attributes = np.ascontiguousarray(cm[:, cm.shape[1] - attributes.shape[1]:])
    return VoxelDownSample(means, out_normals, out_attributes, counts, first, inverse)


# ------------------------------------------------------------------------------------------------------ outlier removal
OutlierRemoval = collections.namedtuple("OutlierRemoval", ["points", "normals", "attributes", "index", "mask", "score",
                                                           "threshold"])


def _pad3(pts):
    """(n, 3): a 2-D cloud gets z = 0, which leaves every squared distance as it is ((dx dx + dy dy) + 0 is exact)."""
    if pts.shape[1] == 3:
        return pts
    return np.ascontiguousarray(np.concatenate([pts, np.zeros((pts.shape[0], 1))], axis=1))


def _filter_inputs(points, normals, attributes):
    pts = _lib.as_cloud(points, "points", (2, 3))
    n, d = pts.shape
    if normals is None and not isinstance(points, np.ndarray) and hasattr(points, "points"):
        own = getattr(points, "normals", None)
        if own is not None and np.ndim(own) == 2 and np.shape(own)[0] == n:
            normals = own
    if normals is not None:
        normals = _as_channel(normals, "normals", n, d)
    if attributes is not None:
        attributes = _as_channel(attributes, "attributes", n, None)
    return pts, normals, attributes


def _kept(pts, normals, attributes, keep, score, threshold):
    index = np.nonzero(keep)[0].astype(np.int32)
    rows = [None if a is None else np.ascontiguousarray(a[index]) for a in (pts, normals, attributes)]
    return OutlierRemoval(rows[0], rows[1], rows[2], index, keep, score, threshold)


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=2.0, normals=None, attributes=None, device=None):
    """Open3D's ``remove_statistical_outlier``: drop the points whose mean distance to their ``nb_neighbors`` nearest
    neighbours is far above the cloud's average (the exact k-NN search and the sums run on the GPU).

    ``a_i`` is the mean distance from point ``i`` to the ``min(nb_neighbors, n)`` nearest points of the cloud, the point
    itself being one of them (Open3D's convention); ``mu`` and ``s`` are the mean and the sample standard deviation of the
    ``a_i``; ``thr = mu + std_ratio s``; point ``i`` is kept iff ``a_i <= thr``.

    Deviation from Open3D (as its behaviour is remembered, not verified against its source): Open3D keeps ``0 < a_i < thr``.
    Under that rule a cloud whose ``a_i`` are all equal, or a point with ``nb_neighbors`` coincident copies, is removed
    entirely; here such points are kept.

    Args:
        points: (n, 2) or (n, 3) array, or anything with ``.points`` (its ``.normals`` ride along when ``normals`` is None).
        nb_neighbors: 1 .. 64.
        std_ratio: >= 0, finite.
        normals, attributes: (n, d) / (n, c) rows that follow the kept points.
    Returns:
        ``OutlierRemoval(points, normals, attributes, index (kept rows, int32), mask (n,) bool, score (n,): a_i,
        threshold: (mu, s, thr))``.
    """
    from . import icp

    pts, normals, attributes = _filter_inputs(points, normals, attributes)
    k = icp._check_k(nb_neighbors, "nb_neighbors")
    ratio = icp._number(std_ratio, "std_ratio")
    if not (np.isfinite(ratio) and ratio >= 0.0):
        raise ValueError("std_ratio must be a finite number >= 0, got %r" % (std_ratio,))
    _single_process("remove_statistical_outlier")
    cloud = _pad3(pts)
    plan = icp.IcpPlan(device)
    try:
        plan.set_target(cloud)
        plan.set_source(cloud)
        keep, score, threshold = plan._outlier_statistical(k, ratio)
    finally:
        plan.close()
    return _kept(pts, normals, attributes, keep, score, threshold)


def remove_radius_outlier(points, nb_points, radius, normals=None, attributes=None, device=None):
    """Open3D's ``remove_radius_outlier``: point ``i`` is kept iff more than ``nb_points`` points of the cloud, the point
    itself included (Open3D's convention), lie within ``radius`` of it (``d2 <= radius radius``).

    Args:
        points, normals, attributes: as in ``remove_statistical_outlier``.
        nb_points: integer >= 0.
        radius: finite, > 0.
    Returns:
        ``OutlierRemoval(points, normals, attributes, index, mask, score (n,) int32: the counts, threshold: nb_points)``.
    """
    from . import icp

    pts, normals, attributes = _filter_inputs(points, normals, attributes)
    nb = icp._number(nb_points, "nb_points")
    if not (np.isfinite(nb) and nb == int(nb) and 0 <= nb < 2 ** 31):
        raise ValueError("nb_points must be an integer >= 0, got %r" % (nb_points,))
    r = icp._check_radius(radius, "radius", False)
    _single_process("remove_radius_outlier")
    cloud = _pad3(pts)
    plan = icp.IcpPlan(device)
    try:
        plan.set_target(cloud)
        plan.set_source(cloud)
        keep, counts = plan._outlier_radius(int(nb), r)
    finally:
        plan.close()
    return _kept(pts, normals, attributes, keep, counts, int(nb))


# ------------------------------------------------------------------------------------------------------------ clustering
class DbscanResult(collections.namedtuple("DbscanResult", ["labels", "core", "counts", "n_clusters", "sizes"])):
    """``labels (n,) int32`` (-1: noise), ``core (n,) bool``, ``counts (n,) int32`` (the neighbours within ``eps``, the point
    itself included), ``n_clusters`` and ``sizes (n_clusters,) int32`` (core and border points of every cluster)."""
    __slots__ = ()

    def clusters(self, min_size=1):
        """The clusters with at least ``min_size`` members as ascending int32 index arrays, in label order: one cloud per
        object for ``cpd.registration_cpd_batch([model] * len(c), [scene[i] for i in c], "rigid")``."""
        order = np.argsort(self.labels, kind="stable")  # noise first, then cluster by cluster, ascending inside each
        ends = np.cumsum(self.sizes, dtype=np.int64) + (self.labels.shape[0] - int(np.sum(self.sizes, dtype=np.int64)))
        return [np.ascontiguousarray(order[e - s:e], dtype=np.int32) for s, e in zip(self.sizes.tolist(), ends.tolist())
                if s >= min_size]


def _check_min_points(v):
    try:
        bad = isinstance(v, (bool, np.bool_, str, bytes)) or not np.isfinite(float(v)) or float(v) != int(v)
    except (TypeError, ValueError, OverflowError):
        bad = True
    if bad or not 1 <= int(v) < 2 ** 31:
        raise ValueError("min_points must be an integer in 1 .. 2^31 - 1, got %r" % (v,))
    return int(v)


def cluster_dbscan(points, eps, min_points, device=None):
    """Open3D's ``cluster_dbscan(eps, min_points)``: split a cloud into its density-connected objects and mark the stray
    points between them as noise (neighbour counts, union-find and numbering run on the GPU).

    ``counts_i`` is the number of points with ``d2 <= eps eps``, the point itself included; point ``i`` is core iff
    ``counts_i >= min_points`` (Open3D's and scikit-learn's convention).  The clusters are the connected components of the
    core points under ``d2 <= eps eps``, numbered 0, 1, ... in ascending order of their smallest core index, which is the
    numbering of a sequential scan: core labels equal scikit-learn's.  A point that is not core but has a core point within
    ``eps`` is a border point; every other point is noise, label -1.

    Deviation from Open3D and scikit-learn (their rule as it is remembered, not verified against their sources): there a
    border point within reach of two clusters goes to the one whose scan reaches it first, which depends on the order of
    the points; here it goes to the cluster of its nearest core neighbour, the minimum of ``(d2, index)``.  Core set, core
    labels and noise are the same.

    The result is byte-identical from run to run and does not depend on the search grid.

    Args:
        points: (n, 2) or (n, 3) array, or anything with ``.points``.
        eps: finite, > 0.
        min_points: integer in 1 .. 2^31 - 1.
    Returns:
        ``DbscanResult(labels, core, counts, n_clusters, sizes)``; ``result.clusters(min_size)`` lists the index arrays.
    """
    from . import icp

    pts, _, _ = _filter_inputs(points, None, None)
    r = icp._check_radius(eps, "eps", False)
    mp = _check_min_points(min_points)
    _single_process("cluster_dbscan")
    cloud = _pad3(pts)
    plan = icp.IcpPlan(device)
    try:
        plan.set_target(cloud)
        plan.set_source(cloud)
        return DbscanResult(*plan._dbscan(r, mp))
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------------- plane segmentation
PlaneSegmentation = collections.namedtuple("PlaneSegmentation", ["plane", "point", "inliers", "mask", "distance", "fitness",
                                                                 "inlier_rmse", "hypothesis", "n_valid", "count", "sum"])
PlaneSet = collections.namedtuple("PlaneSet", ["planes", "points", "labels", "sizes", "n_planes"])

MAX_HYPOTHESES = 1 << 24


def _check_tau(v):
    try:
        tau = float("nan") if isinstance(v, (bool, str, bytes)) else float(v)
    except (TypeError, ValueError):
        tau = float("nan")
    if not (np.isfinite(tau) and tau >= 0.0):
        raise ValueError("distance_threshold must be a finite number >= 0, got %r" % (v,))
    return tau


def _check_count(v, name, lo, hi):
    try:
        bad = isinstance(v, (bool, np.bool_, str, bytes)) or not np.isfinite(float(v)) or float(v) != int(v)
    except (TypeError, ValueError, OverflowError):
        bad = True
    if bad or not lo <= int(v) <= hi:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, v))
    return int(v)


def _cos_theta(max_normal_angle, have_normals):
    """cos of the angle for the library, -1.0 for "no normal test"."""
    if max_normal_angle is None:
        return -1.0
    if not have_normals:
        raise ValueError("max_normal_angle needs normals")
    try:
        a = float("nan") if isinstance(max_normal_angle, (bool, str, bytes)) else float(max_normal_angle)
    except (TypeError, ValueError):
        a = float("nan")
    if not (np.isfinite(a) and 0.0 <= a <= np.pi / 2.0):
        raise ValueError("max_normal_angle must lie in [0, pi / 2] (radians), got %r" % (max_normal_angle,))
    return max(0.0, float(np.cos(a)))


def _plane_row(plane):
    plane = np.ascontiguousarray(plane, dtype=np.float64).reshape(-1)
    if plane.shape[0] != 6 or not np.all(np.isfinite(plane)):
        raise ValueError("a plane is six finite numbers (unit normal, anchor)")
    return plane


class PlanePlan(_lib.Handle):
    """One ``prg_plane`` handle: a 3-D cloud (with or without normals) on one device / stream and the stages of the plane
    search, each of which can be driven on its own.  A plane is six numbers: the unit normal and the anchor the distances
    are taken from.  ``cos_theta`` is the cosine of the largest angle between a point's normal and the plane's, ``None``
    for no normal test."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_plane_create, _lib.lib.prg_plane_destroy, device)
        self.n = 0
        self.n_hyp = 0
        self.have_normals = False

    @staticmethod
    def _cos(cos_theta):
        return -1.0 if cos_theta is None else float(cos_theta)

    def set_points(self, points, normals=None):
        points = _lib.as_cloud(points, "points", (3,), 3)
        if normals is not None:
            normals = _as_channel(normals, "normals", points.shape[0], 3)
        _lib.check(_lib.lib.prg_plane_set_points(self._h, _lib.ptr(points), _lib.ptr(normals), points.shape[0]))
        self.n = points.shape[0]
        self.have_normals = normals is not None

    def count(self):
        """The points of the handle's cloud: those of ``set_points`` less what ``remove`` has dropped."""
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib.prg_plane_count(self._h, ctypes.byref(n)))
        return int(n.value)

    def build(self, seed, n_hypotheses, offset=0):
        """Hypotheses ``offset .. offset + n_hypotheses - 1`` of the stream ``seed``."""
        _lib.check(_lib.lib.prg_plane_build(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), int(n_hypotheses)))
        self.n_hyp = int(n_hypotheses)

    def hypotheses(self, triples=True):
        """(triples (H, 3) int32 or None, planes (H, 6), valid (H,) bool)."""
        tri = np.empty((self.n_hyp, 3), dtype=np.int32) if triples else None
        planes = np.empty((self.n_hyp, 6))
        valid = np.empty(self.n_hyp, dtype=np.int32)
        _lib.check(_lib.lib.prg_plane_get_hypotheses(self._h, _lib.ptr(tri), _lib.ptr(planes), _lib.ptr(valid)))
        return tri, planes, valid != 0

    def set_hypotheses(self, planes, valid):
        planes = np.ascontiguousarray(planes, dtype=np.float64)
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        if planes.ndim != 2 or planes.shape[1] != 6 or valid.shape != (planes.shape[0],):
            raise ValueError("planes must be (H, 6) and valid (H,), got %s and %s" % (planes.shape, valid.shape))
        if not np.all(np.isfinite(planes)):
            raise ValueError("planes contains NaN or infinity")
        _lib.check(_lib.lib.prg_plane_set_hypotheses(self._h, _lib.ptr(planes), _lib.ptr(valid), planes.shape[0]))
        self.n_hyp = planes.shape[0]

    def score(self, tau, cos_theta=None):
        _lib.check(_lib.lib.prg_plane_score(self._h, _check_tau(tau), self._cos(cos_theta)))

    def scores(self):
        """(count (H,) int32 with -1 for an invalid hypothesis, sum (H,))."""
        cnt = np.empty(self.n_hyp, dtype=np.int32)
        sm = np.empty(self.n_hyp)
        _lib.check(_lib.lib.prg_plane_get_scores(self._h, _lib.ptr(cnt), _lib.ptr(sm)))
        return cnt, sm

    def best(self):
        """(index, n_valid, count, sum, plane (6,)) of the winner; index -1 when no hypothesis is valid."""
        idx, nv, cnt, sm = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0.0)
        plane = np.empty(6)
        _lib.check(_lib.lib.prg_plane_best(self._h, ctypes.byref(idx), ctypes.byref(nv), ctypes.byref(cnt), ctypes.byref(sm),
                                           _lib.ptr(plane)))
        return int(idx.value), int(nv.value), int(cnt.value), float(sm.value), plane

    def refine(self, plane, tau, iters=3, cos_theta=None):
        """(plane (6,), sums (iters, 10)) after ``iters`` refits that start from ``plane``; row i of ``sums`` holds the
        inlier count, the sums of ``q = x - a`` and of ``q q^T`` (xx, xy, xz, yy, yz, zz) of iteration i."""
        plane = _plane_row(plane).copy()
        iters = _check_count(iters, "iters", 0, 1000)
        trace = np.zeros((iters, 10))
        _lib.check(_lib.lib.prg_plane_refine(self._h, _check_tau(tau), self._cos(cos_theta), iters, _lib.ptr(plane),
                                             _lib.ptr(trace) if iters else None))
        return plane, trace

    def classify(self, plane, tau, cos_theta=None):
        """(mask (n,) bool, signed distance (n,), count, sum of the squared inlier distances) of ``plane``."""
        plane = _plane_row(plane)
        n = self.count()
        mask = np.empty(n, dtype=np.int32)
        dist = np.empty(n)
        cnt, sm = ctypes.c_int(0), ctypes.c_double(0.0)
        _lib.check(_lib.lib.prg_plane_classify(self._h, _lib.ptr(plane), _check_tau(tau), self._cos(cos_theta), _lib.ptr(mask),
                                               _lib.ptr(dist), ctypes.byref(cnt), ctypes.byref(sm)))
        return mask != 0, dist, int(cnt.value), float(sm.value)

    def remove(self):
        """Drops the inliers of the last ``classify``; the rest stays on the device in ascending index.  Returns how many
        points are left."""
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib.prg_plane_remove(self._h, ctypes.byref(n)))
        return int(n.value)

    def segment(self, tau, num_iterations, seed, refine_iters, cos_theta=None, offset=0):
        """All stages on the handle's cloud: a ``PlaneSegmentation`` whose indices are rows of that cloud."""
        n = self.count()
        self.build(seed, num_iterations, offset)
        self.score(tau, cos_theta)
        idx, n_valid, cnt, sm, plane = self.best()
        if idx < 0:
            return PlaneSegmentation(None, None, np.zeros(0, dtype=np.int32), np.zeros(n, dtype=bool), np.zeros(n), 0.0, 0.0,
                                     -1, n_valid, 0, 0.0)
        plane, _ = self.refine(plane, tau, refine_iters, cos_theta)
        mask, dist, k, total = self.classify(plane, tau, cos_theta)
        nrm, a = plane[:3], plane[3:]
        abcd = np.array([nrm[0], nrm[1], nrm[2], -((nrm[0] * a[0] + nrm[1] * a[1]) + nrm[2] * a[2])])
        return PlaneSegmentation(abcd, a.copy(), np.nonzero(mask)[0].astype(np.int32), mask, dist, k / float(n),
                                 float(np.sqrt(total / k)) if k else 0.0, idx, n_valid, cnt, sm)


def _plane_inputs(points, normals, distance_threshold, num_iterations, refine_iters, max_normal_angle, what):
    pts = _lib.as_cloud(points, "points", (3,), 3)
    if normals is None and max_normal_angle is not None and not isinstance(points, np.ndarray) and hasattr(points, "points"):
        own = getattr(points, "normals", None)
        if own is not None and np.ndim(own) == 2 and np.shape(own)[0] == pts.shape[0]:
            normals = own
    if normals is not None:
        normals = _as_channel(normals, "normals", pts.shape[0], 3)
    tau = _check_tau(distance_threshold)
    n_hyp = _check_count(num_iterations, "num_iterations", 1, MAX_HYPOTHESES)
    iters = _check_count(refine_iters, "refine_iters", 0, 1000)
    cos_theta = _cos_theta(max_normal_angle, normals is not None)
    _single_process(what)
    return pts, (normals if cos_theta >= 0.0 else None), tau, n_hyp, iters, (cos_theta if cos_theta >= 0.0 else None)


def segment_plane(points, distance_threshold, num_iterations=1000, seed=0, refine_iters=3, normals=None,
                  max_normal_angle=None, device=None, hypothesis_offset=0):
    """Open3D's ``segment_plane(distance_threshold, ransac_n=3, num_iterations)``: the plane that most points of a cloud lie
    within ``distance_threshold`` of - the table or floor a scene stands on, to be taken out before ``cluster_dbscan``
    (the draws, the sweep hypotheses x points, the winner and the refits run on the GPU in fp64).

    Hypothesis ``h`` is the plane through three points drawn by a counter-based generator from ``seed`` (so the result does
    not depend on how the work is cut); its score is the number of points with ``|dist| <= distance_threshold`` and the sum
    of their squared distances; the winner (most inliers, then the smaller sum, then the smaller ``h``) is refitted
    ``refine_iters`` times by least squares on its inliers.  Distances are taken from an anchor point on the plane, never
    as ``n . x + d``, so a cloud far from the origin loses nothing.  The result is byte-identical from run to run.

    Deviations from Open3D (its behaviour as it is remembered, not verified against its source): a point exactly at the
    threshold is an inlier (Open3D: ``<``); the draws are this module's own; ``ransac_n`` is 3 and there is no
    ``probability`` early stop; the final plane is refitted more than once.

    Args:
        points: (n, 3) array with n >= 3, or anything with ``.points`` (its ``.normals`` are used when ``max_normal_angle`` is
            given and ``normals`` is None).
        distance_threshold: finite, >= 0.
        num_iterations: the number of hypotheses, 1 .. 2^24.
        seed: of the draws.
        refine_iters: least-squares refits of the winner, 0 .. 1000.
        normals, max_normal_angle: with both, an inlier's normal ``m`` must also lie within ``max_normal_angle`` (radians,
            0 .. pi / 2) of the plane's, either way round: ``|n . m| >= cos(max_normal_angle) |m|``.  A zero normal never
            passes.  ``max_normal_angle`` without normals is a ``ValueError``.
        hypothesis_offset: the first hypothesis of the stream (``segment_planes`` gives round k the offset
            ``k num_iterations``).
    Returns:
        ``PlaneSegmentation(plane (a, b, c, d) with unit (a, b, c) whose component of largest magnitude is positive and
        d = -n . point, point (3,): the anchor, inliers (ascending int32), mask (n,) bool, distance (n,): signed, to the final
        plane, fitness = len(inliers) / n, inlier_rmse, hypothesis, n_valid, count, sum)``; the last four describe the
        RANSAC winner before the refit.  When no hypothesis is valid (no three distinct, non-collinear points were drawn)
        ``plane`` and ``point`` are None, ``inliers`` is empty and ``hypothesis`` is -1.
    """
    pts, normals, tau, n_hyp, iters, cos_theta = _plane_inputs(points, normals, distance_threshold, num_iterations,
                                                               refine_iters, max_normal_angle, "segment_plane")
    offset = _check_count(hypothesis_offset, "hypothesis_offset", 0, 2 ** 62)
    plan = PlanePlan(device)
    try:
        plan.set_points(pts, normals)
        return plan.segment(tau, n_hyp, seed, iters, cos_theta, offset)
    finally:
        plan.close()


def segment_planes(points, distance_threshold, max_planes, min_inliers=3, num_iterations=1000, seed=0, refine_iters=3,
                   normals=None, max_normal_angle=None, device=None):
    """Up to ``max_planes`` planes, one after the other: by definition ``segment_plane`` on the points that no earlier plane
    has taken, kept in ascending original index, round ``k`` with ``hypothesis_offset = k num_iterations``.  It stops after
    ``max_planes`` rounds, when a round's final inlier count is below ``min_inliers`` (that plane is dropped), when a round
    has no valid hypothesis, or when fewer than three points are left.  The remaining cloud stays on the device between the
    rounds and shrinks, so later rounds sweep fewer points.

    Returns:
        ``PlaneSet(planes (P, 4), points (P, 3): the anchors, labels (n,) int32: the plane of every point, -1 for the rest,
        sizes (P,) int32, n_planes)``.
    """
    pts, normals, tau, n_hyp, iters, cos_theta = _plane_inputs(points, normals, distance_threshold, num_iterations,
                                                               refine_iters, max_normal_angle, "segment_planes")
    rounds = _check_count(max_planes, "max_planes", 0, 2 ** 31 - 1)
    least = _check_count(min_inliers, "min_inliers", 0, 2 ** 31 - 1)
    labels = np.full(pts.shape[0], -1, dtype=np.int32)
    left = np.arange(pts.shape[0])
    planes, anchors, sizes = [], [], []
    plan = PlanePlan(device)
    try:
        plan.set_points(pts, normals)
        for k in range(rounds):
            if left.shape[0] < 3:
                break
            seg = plan.segment(tau, n_hyp, seed, iters, cos_theta, k * n_hyp)
            if seg.hypothesis < 0 or seg.inliers.shape[0] < least:
                break
            labels[left[seg.mask]] = k
            planes.append(seg.plane)
            anchors.append(seg.point)
            sizes.append(seg.inliers.shape[0])
            left = left[~seg.mask]
            if plan.remove() != left.shape[0]:
                raise _lib.ProbregHipError("segment_planes: the device kept %d points, the host %d" % (plan.count(), left.shape[0]))
    finally:
        plan.close()
    return PlaneSet(np.array(planes, dtype=np.float64).reshape(-1, 4), np.array(anchors, dtype=np.float64).reshape(-1, 3),
                    labels, np.array(sizes, dtype=np.int32), len(planes))
