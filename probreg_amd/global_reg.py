"""Global registration: a start pose from matched descriptors, for clouds that are turned too far for the local methods.

The reference has no counterpart; its examples get the start pose from Open3D (``compute_fpfh_feature``, then
``registration_ransac_based_on_feature_matching``).  Here both hot paths run in ``libprobreg_hip.so``
(``prg_feature_match*``, ``prg_ransac_*``, csrc/global_reg.hip) in fp64: the all-pairs nearest-descriptor sweep and the
sweep "hypotheses x correspondences".  DESIGN.md section 3.13 is the definition; results are byte-identical from run to run.
Open3D is not imported.

The result plugs straight into the local methods::

    from probreg_amd import cpd, filterreg, global_reg
    res = global_reg.registration_global(source, target, max_distance=0.08)
    init = dict(rot=res.transformation.rot, t=res.transformation.t)
    tf = cpd.registration_cpd(source, target, tf_init_params=init).transformation
    tf = filterreg.registration_filterreg(source, target, sigma2=None, tf_init_params=init).transformation

Stages, each of which can be driven and read on its own (``RansacPlan``):
  * ``feature_matching``: nearest descriptor per source row, optionally kept only when mutual;
  * ``build``: hypothesis ``h`` draws three correspondences by splitmix64 on the counters ``3h + 1 .. 3h + 3``, is checked
    (distinct, Open3D's edge-length check, non-degenerate triangle) and gets the Kabsch pose of its three pairs;
  * ``score``: inlier count and ordered sum of squared residuals per hypothesis; the winner has the largest count, then the
    smallest sum, then the smallest index;
  * ``refine``: Kabsch over the inliers of the current pose, repeated.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from . import dist as pdist
from .engine import _current_device_and_stream
from .transformation import RigidTransformation

MAX_DIM = 64

GlobalResult = collections.namedtuple("GlobalResult", ["transformation", "fitness", "inlier_rmse", "inliers"])


def _as_rows(a, name, cols=None):
    a = np.ascontiguousarray(np.asarray(getattr(a, "points", a)), dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1 or (cols is not None and a.shape[1] != cols):
        raise ValueError("%s must be (n, %s) with n >= 1, got shape %s" % (name, "d" if cols is None else cols, a.shape))
    if not np.all(np.isfinite(a)):
        raise ValueError("%s contains NaN or infinity" % name)
    return a


def _single_process(what):
    if pdist.world()[1] > 1:
        raise NotImplementedError("%s: sharding over %d ranks is not supported; run it in one process."
                                  % (what, pdist.world()[1]))


def _match_raw(fa, fb, mutual, segments, device):
    fa, fb = _as_rows(fa, "source_feature"), _as_rows(fb, "target_feature")
    if fa.shape[1] != fb.shape[1]:
        raise ValueError("descriptor dimensions differ: source %d, target %d" % (fa.shape[1], fb.shape[1]))
    if not 1 <= fa.shape[1] <= MAX_DIM:
        raise ValueError("descriptor dimension must lie in 1 .. %d, got %d" % (MAX_DIM, fa.shape[1]))
    _single_process("feature_matching")
    _lib.require_gpu()
    dev, st = _current_device_and_stream(device)
    idx = np.empty(fa.shape[0], dtype=np.int32)
    d2 = np.empty(fa.shape[0])
    if mutual:
        keep = np.empty(fa.shape[0], dtype=np.int32)
        _lib.check(_lib.lib.prg_feature_match_mutual(dev, ctypes.c_void_p(st), _lib.ptr(fa), fa.shape[0], _lib.ptr(fb),
                                                     fb.shape[0], fa.shape[1], int(segments), _lib.ptr(idx), _lib.ptr(d2),
                                                     _lib.ptr(keep)))
        return idx, d2, keep != 0
    _lib.check(_lib.lib.prg_feature_match(dev, ctypes.c_void_p(st), _lib.ptr(fa), fa.shape[0], _lib.ptr(fb), fb.shape[0],
                                          fa.shape[1], int(segments), _lib.ptr(idx), _lib.ptr(d2)))
    return idx, d2, np.ones(fa.shape[0], dtype=bool)


def nearest_feature(source_feature, target_feature, segments=0, device=None):
    """(index (na,) int32, d2 (na,)): for every source row the target row of least squared distance, summed over the
    columns in ascending order; ties go to the smaller index.  ``segments`` cuts the sweep (0: automatic) and does not
    change the result."""
    idx, d2, _ = _match_raw(source_feature, target_feature, False, segments, device)
    return idx, d2


def feature_matching(source_feature, target_feature, mutual=True, segments=0, device=None):
    """(pairs (C, 2) int32 of (source index, target index) ascending in the source index, d2 (C,)).  ``mutual`` keeps a pair
    only when the source row is the best match of its target row as well."""
    idx, d2, keep = _match_raw(source_feature, target_feature, bool(mutual), segments, device)
    src = np.nonzero(keep)[0].astype(np.int32)
    return np.stack([src, idx[src]], axis=1).astype(np.int32), d2[src]


def _check_tau(tau):
    if not (np.isfinite(tau) and tau >= 0.0):
        raise ValueError("max_distance must be finite and >= 0, got %r" % (tau,))
    return float(tau)


class RansacPlan(_lib.Handle):
    """One ``prg_ransac`` handle: correspondences on one device / stream and the stages of the pose search."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_ransac_create, _lib.lib.prg_ransac_destroy, device)
        self.n_corr = 0
        self.n_hyp = 0

    def set_correspondences(self, p, q):
        """Source points ``p`` (C, 3) and their matched target points ``q`` (C, 3)."""
        p, q = _as_rows(p, "p", 3), _as_rows(q, "q", 3)
        if p.shape != q.shape:
            raise ValueError("p and q must have the same shape, got %s and %s" % (p.shape, q.shape))
        _lib.check(_lib.lib.prg_ransac_set_correspondences(self._h, _lib.ptr(p), _lib.ptr(q), p.shape[0]))
        self.n_corr = p.shape[0]

    def build(self, seed, n_hypotheses, edge_similarity=0.9, offset=0):
        """Hypotheses ``offset .. offset + n_hypotheses - 1`` of the stream ``seed``."""
        _lib.check(_lib.lib.prg_ransac_build(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset), int(n_hypotheses),
                                             float(edge_similarity)))
        self.n_hyp = int(n_hypotheses)

    def hypotheses(self, triples=True):
        """(triples (H, 3) int32 or None, pose (H, 12) = rotation row-major then shift, valid (H,) bool)."""
        tri = np.empty((self.n_hyp, 3), dtype=np.int32) if triples else None
        pose = np.empty((self.n_hyp, 12))
        valid = np.empty(self.n_hyp, dtype=np.int32)
        _lib.check(_lib.lib.prg_ransac_get_hypotheses(self._h, _lib.ptr(tri), _lib.ptr(pose), _lib.ptr(valid)))
        return tri, pose, valid != 0

    def set_hypotheses(self, pose, valid):
        pose = np.ascontiguousarray(pose, dtype=np.float64)
        valid = np.ascontiguousarray(valid, dtype=np.int32)
        if pose.ndim != 2 or pose.shape[1] != 12 or valid.shape != (pose.shape[0],):
            raise ValueError("pose must be (H, 12) and valid (H,), got %s and %s" % (pose.shape, valid.shape))
        if not np.all(np.isfinite(pose)):
            raise ValueError("pose contains NaN or infinity")
        _lib.check(_lib.lib.prg_ransac_set_hypotheses(self._h, _lib.ptr(pose), _lib.ptr(valid), pose.shape[0]))
        self.n_hyp = pose.shape[0]

    def score(self, tau):
        _lib.check(_lib.lib.prg_ransac_score(self._h, _check_tau(tau)))

    def scores(self):
        """(count (H,) int32 with -1 for an invalid hypothesis, sum (H,))."""
        cnt = np.empty(self.n_hyp, dtype=np.int32)
        sm = np.empty(self.n_hyp)
        _lib.check(_lib.lib.prg_ransac_get_scores(self._h, _lib.ptr(cnt), _lib.ptr(sm)))
        return cnt, sm

    def best(self):
        """(index, count, sum, pose (12,)) of the winner; ``ProbregHipError`` when no hypothesis is valid."""
        idx, cnt, sm = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0.0)
        pose = np.empty(12)
        _lib.check(_lib.lib.prg_ransac_best(self._h, ctypes.byref(idx), ctypes.byref(cnt), ctypes.byref(sm), _lib.ptr(pose)))
        return int(idx.value), int(cnt.value), float(sm.value), pose

    def refine(self, pose, tau, iters=3):
        """(pose (12,), count, sum, inlier flags (C,) bool) after ``iters`` refits that start from ``pose``."""
        pose = np.array(pose, dtype=np.float64).reshape(12)
        cnt, sm = ctypes.c_int(0), ctypes.c_double(0.0)
        inl = np.empty(self.n_corr, dtype=np.int32)
        _lib.check(_lib.lib.prg_ransac_refine(self._h, _check_tau(tau), int(iters), _lib.ptr(pose), ctypes.byref(cnt),
                                              ctypes.byref(sm), _lib.ptr(inl)))
        return pose, int(cnt.value), float(sm.value), inl != 0


def registration_ransac(source, target, correspondences, max_distance, n_hypotheses=65536, edge_similarity=0.9,
                        refine_iters=3, seed=0, device=None):
    """The rigid pose (no scale) that most ``correspondences`` (C, 2) of (source index, target index) agree on within
    ``max_distance``: ``GlobalResult(transformation, fitness, inlier_rmse, inliers)`` with ``fitness = inliers / C``,
    ``inlier_rmse`` over them and ``inliers`` the indices into ``correspondences``, all at the final pose."""
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    corr = np.asarray(correspondences)
    if corr.ndim != 2 or corr.shape[1] != 2 or not np.issubdtype(corr.dtype, np.integer):
        raise ValueError("correspondences must be an integer array of shape (C, 2), got %s %s" % (corr.dtype, corr.shape))
    if corr.shape[0] < 3:
        raise ValueError("need at least 3 correspondences, got %d" % corr.shape[0])
    if corr.min() < 0 or corr[:, 0].max() >= src.shape[0] or corr[:, 1].max() >= tgt.shape[0]:
        raise ValueError("correspondences index outside the clouds")
    tau = _check_tau(max_distance)
    if int(n_hypotheses) != n_hypotheses or n_hypotheses < 1:
        raise ValueError("n_hypotheses must be an integer >= 1, got %r" % (n_hypotheses,))
    if not 0.0 <= edge_similarity <= 1.0:
        raise ValueError("edge_similarity must lie in [0, 1], got %r" % (edge_similarity,))
    if int(refine_iters) != refine_iters or refine_iters < 0:
        raise ValueError("refine_iters must be an integer >= 0, got %r" % (refine_iters,))
    _single_process("registration_ransac")
    plan = RansacPlan(device)
    try:
        plan.set_correspondences(src[corr[:, 0]], tgt[corr[:, 1]])
        plan.build(seed, n_hypotheses, edge_similarity)
        plan.score(tau)
        _, _, _, pose = plan.best()
        pose, cnt, sm, inl = plan.refine(pose, tau, refine_iters)
    finally:
        plan.close()
    tf = RigidTransformation(pose[:9].reshape(3, 3).copy(), pose[9:].copy(), 1.0)
    return GlobalResult(tf, cnt / float(corr.shape[0]), float(np.sqrt(sm / cnt)) if cnt else 0.0, np.nonzero(inl)[0])


def registration_global(source, target, feature_fn=None, max_distance=0.05, mutual=True, voxel_size=None, **ransac_kwargs):
    """Descriptors of both clouds (default ``fpfh.FPFH()``), their matches, then ``registration_ransac``.  ``source`` and
    ``target`` are (n, 3) arrays or anything with ``.points``.

    ``voxel_size``: when given, both clouds go through ``preprocess.voxel_down_sample(cloud, voxel_size)`` first, and
    descriptors, matching and the pose search run on the down-sampled clouds (FPFH stops being discriminative on dense
    clouds).  ``fitness`` and ``inliers`` of the result then refer to the down-sampled clouds and their correspondences, not
    to the rows of ``source`` and ``target``; the pose holds for the full clouds all the same."""
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    _check_tau(max_distance)
    _single_process("registration_global")
    device = ransac_kwargs.get("device")
    if voxel_size is not None:
        from . import preprocess
        voxel_size = preprocess._check_voxel_size(voxel_size)
        src = preprocess.voxel_down_sample(src, voxel_size, device=device).points
        tgt = preprocess.voxel_down_sample(tgt, voxel_size, device=device).points
    if feature_fn is None:
        from . import fpfh
        feature_fn = fpfh.FPFH()
    pairs, _ = feature_matching(feature_fn(src), feature_fn(tgt), mutual, device=device)
    if pairs.shape[0] < 3:
        raise ValueError("fewer than 3 correspondences are left after matching (%d)" % pairs.shape[0])
    return registration_ransac(src, tgt, pairs, max_distance, **ransac_kwargs)
