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

``registration_fgr`` (``FgrPlan``, ``prg_fgr_*``, csrc/fgr.hip) is the second estimator, for
correspondences that are mostly wrong: fast global registration (Zhou, Park, Koltun, ECCV 2016) samples no poses; it runs
Gauss-Newton over all pairs at once under a Geman-McClure line process whose scale is annealed, after a tuple test that
removes most wrong matches.  It is deterministic and needs no hypothesis budget.
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
FgrResult = collections.namedtuple("FgrResult", ["transformation", "fitness", "inlier_rmse", "inliers", "used", "weights", "mu",
                                                 "n_iter", "n_tuples", "n_trials", "status"])
FgrState = collections.namedtuple("FgrState", ["pose", "mu", "n_iter", "status", "objective"])
FGR_STATUS = ("ok", "too_few", "degenerate")
FGR_MAX_CORRESPONDENCES = 2 ** 31 // 100   # the trial counter 100 C and the draw stay in range
FGR_IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)


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


class FgrPlan(_lib.Handle):
    """One ``prg_fgr`` handle: two clouds and their correspondences on one device / stream and the stages of fast global
    registration.  Poses are 12 doubles (rotation row-major, then the shift) and, but for
    ``state(caller_units=True)``, move the normalised clouds."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_fgr_create, _lib.lib.prg_fgr_destroy, device)
        self.n_corr = 0
        self.n_used = 0
        self.chunk = 0

    def set_clouds(self, source, target):
        src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
        _lib.check(_lib.lib.prg_fgr_set_clouds(self._h, _lib.ptr(src), src.shape[0], _lib.ptr(tgt), tgt.shape[0]))
        self.n_corr = self.n_used = 0

    def set_correspondences(self, corr):
        """(C, 2) integer pairs (source index, target index); ``normalise`` checks them against the clouds."""
        corr = np.ascontiguousarray(corr, dtype=np.int32)
        if corr.ndim != 2 or corr.shape[1] != 2:
            raise ValueError("correspondences must have shape (C, 2), got %s" % (corr.shape,))
        _lib.check(_lib.lib.prg_fgr_set_correspondences(self._h, _lib.ptr(corr), corr.shape[0]))
        self.n_corr = corr.shape[0]
        self.n_used = 0

    def normalise(self, use_absolute_scale=False):
        """(mean_p (3,), mean_q (3,), scale): the means of all source and all target points and the largest distance of a
        point from the mean of its cloud."""
        mp, mq, sc = np.empty(3), np.empty(3), ctypes.c_double(0.0)
        _lib.check(_lib.lib.prg_fgr_normalise(self._h, int(bool(use_absolute_scale)), _lib.ptr(mp), _lib.ptr(mq),
                                              ctypes.byref(sc)))
        return mp, mq, float(sc.value)

    def set_chunk(self, trials):
        """Trials per launch of ``tuples`` (0: the default); changes no result."""
        _lib.check(_lib.lib.prg_fgr_set_chunk(self._h, int(trials)))
        self.chunk = int(trials)

    def tuples(self, seed=0, tuple_scale=0.95, maximum_tuple_count=1000):
        """(used (3 n_tuples,) int32, n_tuples, n_trials); the used pairs are installed."""
        nt, ntr = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib.prg_fgr_tuples(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, float(tuple_scale), int(maximum_tuple_count),
                                           ctypes.byref(nt), ctypes.byref(ntr)))
        self.n_used = 3 * int(nt.value)
        return self.used(), int(nt.value), int(ntr.value)

    def set_used(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        if idx.ndim != 1:
            raise ValueError("the used indices must have shape (K,), got %s" % (idx.shape,))
        _lib.check(_lib.lib.prg_fgr_set_used(self._h, _lib.ptr(idx), idx.shape[0]))
        self.n_used = idx.shape[0]

    def used(self):
        idx = np.empty(self.n_used, dtype=np.int32)
        if self.n_used:
            _lib.check(_lib.lib.prg_fgr_get_used(self._h, _lib.ptr(idx)))
        return idx

    def set_state(self, pose=FGR_IDENTITY, mu=1.0):
        pose = np.array(pose, dtype=np.float64).reshape(12)
        _lib.check(_lib.lib.prg_fgr_set_state(self._h, _lib.ptr(pose), float(mu)))

    def sums(self, pose=None, mu=None):
        """The 28 raw sums (A's upper triangle row-major, g, the objective) at ``pose`` and ``mu`` (default: the state's)."""
        if pose is not None or mu is not None:
            if pose is None or mu is None:
                raise ValueError("give both pose and mu, or neither")
            self.set_state(pose, mu)
        out = np.empty(28)
        _lib.check(_lib.lib.prg_fgr_sums(self._h, _lib.ptr(out)))
        return out

    def step(self, decrease_mu=False, division_factor=1.4, maximum_correspondence_distance=0.025):
        """One step from the last ``sums``; the pose after it."""
        _lib.check(_lib.lib.prg_fgr_step(self._h, int(bool(decrease_mu)), float(division_factor),
                                         float(maximum_correspondence_distance)))
        return self.state().pose

    def iterate(self, n, decrease_mu=True, division_factor=1.4, maximum_correspondence_distance=0.025):
        """``n`` times "sums, step" from the state; the final ``FgrState``."""
        _lib.check(_lib.lib.prg_fgr_iterate(self._h, int(n), int(bool(decrease_mu)), float(division_factor),
                                            float(maximum_correspondence_distance)))
        return self.state()

    def state(self, caller_units=False):
        pose = np.empty(12)
        mu, it, st, obj = ctypes.c_double(0.0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0.0)
        _lib.check(_lib.lib.prg_fgr_get_state(self._h, int(bool(caller_units)), _lib.ptr(pose), ctypes.byref(mu), ctypes.byref(it),
                                              ctypes.byref(st), ctypes.byref(obj)))
        return FgrState(pose, float(mu.value), int(it.value), FGR_STATUS[st.value], float(obj.value))

    def weights(self):
        """The line-process value of every used pair at the state's pose and mu."""
        w = np.empty(self.n_used)
        if self.n_used:
            _lib.check(_lib.lib.prg_fgr_get_weights(self._h, _lib.ptr(w)))
        return w


def _check_correspondences(corr, src, tgt):
    corr = np.asarray(corr)
    if corr.ndim != 2 or corr.shape[1] != 2 or not np.issubdtype(corr.dtype, np.integer):
        raise ValueError("correspondences must be an integer array of shape (C, 2), got %s %s" % (corr.dtype, corr.shape))
    if corr.shape[0] < 3:
        raise ValueError("need at least 3 correspondences, got %d" % corr.shape[0])
    if corr.min() < 0 or corr[:, 0].max() >= src.shape[0] or corr[:, 1].max() >= tgt.shape[0]:
        raise ValueError("correspondences index outside the clouds")
    return corr


def registration_fgr(source, target, correspondences, maximum_correspondence_distance=0.025, iteration_number=64,
                     division_factor=1.4, decrease_mu=True, use_absolute_scale=False, tuple_test=True, tuple_scale=0.95,
                     maximum_tuple_count=1000, seed=0, max_distance=None, device=None):
    """Fast global registration (Open3D's ``registration_fgr_based_on_correspondence``) of ``correspondences`` (C, 2) of
    (source index, target index): ``FgrResult(transformation, fitness, inlier_rmse, inliers, used, weights, mu, n_iter,
    n_tuples, n_trials, status)``.

    ``transformation`` is rigid (no scale) in the caller's units.  ``fitness``, ``inlier_rmse`` and ``inliers`` are taken over
    all correspondences within ``max_distance`` at the final pose, as in ``GlobalResult``; ``max_distance=None`` means
    ``maximum_correspondence_distance`` in the caller's units (times the clouds' scale unless ``use_absolute_scale``).
    ``used`` are the indices into ``correspondences`` the optimisation ran on: three per accepted tuple in acceptance order
    with repeats kept, or ``arange(C)`` without the tuple test; ``weights`` their final line-process values, ``mu`` the final
    scale of the line process.  ``status`` is "ok", "too_few" (fewer than three used pairs: the normalised pose stays the
    identity, so the result only moves the source's mean onto the target's) or "degenerate" (a failed pivot: the pose of
    the last good step)."""
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    corr = _check_correspondences(correspondences, src, tgt)
    if corr.shape[0] > FGR_MAX_CORRESPONDENCES:
        raise ValueError("at most %d correspondences, got %d" % (FGR_MAX_CORRESPONDENCES, corr.shape[0]))
    mcd = _check_tau(maximum_correspondence_distance)
    if int(iteration_number) != iteration_number or iteration_number < 0:
        raise ValueError("iteration_number must be an integer >= 0, got %r" % (iteration_number,))
    if not (np.isfinite(division_factor) and division_factor > 1.0):
        raise ValueError("division_factor must be finite and > 1, got %r" % (division_factor,))
    if not 0.0 < tuple_scale <= 1.0:
        raise ValueError("tuple_scale must lie in (0, 1], got %r" % (tuple_scale,))
    if int(maximum_tuple_count) != maximum_tuple_count or maximum_tuple_count < 1:
        raise ValueError("maximum_tuple_count must be an integer >= 1, got %r" % (maximum_tuple_count,))
    if max_distance is not None:
        max_distance = _check_tau(max_distance)
    _single_process("registration_fgr")
    plan = FgrPlan(device)
    try:
        plan.set_clouds(src, tgt)
        plan.set_correspondences(corr)
        _, _, scale = plan.normalise(use_absolute_scale)
        if not scale > 0.0:
            raise ValueError("both clouds are a single point: there is nothing to register")
        if tuple_test:
            used, n_tuples, n_trials = plan.tuples(seed, tuple_scale, maximum_tuple_count)
        else:
            used, n_tuples, n_trials = np.arange(corr.shape[0], dtype=np.int32), 0, 0
            plan.set_used(used)
        plan.set_state(FGR_IDENTITY, scale if use_absolute_scale else 1.0)
        st = plan.iterate(int(iteration_number), decrease_mu, division_factor, mcd)
        weights = plan.weights()
        pose = plan.state(caller_units=True).pose
    finally:
        plan.close()
    status = "too_few" if used.shape[0] < 3 else st.status
    tau = max_distance if max_distance is not None else mcd * (1.0 if use_absolute_scale else scale)
    ev = RansacPlan(device)
    try:
        ev.set_correspondences(src[corr[:, 0]], tgt[corr[:, 1]])
        pose, cnt, sm, inl = ev.refine(pose, tau, 0)
    finally:
        ev.close()
    tf = RigidTransformation(pose[:9].reshape(3, 3).copy(), pose[9:].copy(), 1.0)
    return FgrResult(tf, cnt / float(corr.shape[0]), float(np.sqrt(sm / cnt)) if cnt else 0.0, np.nonzero(inl)[0], used, weights,
                     st.mu, st.n_iter, n_tuples, n_trials, status)


def registration_global(source, target, feature_fn=None, max_distance=0.05, mutual=True, voxel_size=None, method="ransac",
                        **kwargs):
    """Descriptors of both clouds (default ``fpfh.FPFH()``), their matches, then ``registration_ransac``
    (``method="ransac"``, the default) or ``registration_fgr`` (``method="fgr"``), which gets ``kwargs``; the result is a
    ``GlobalResult`` either way.  ``source`` and ``target`` are (n, 3) arrays or anything with ``.points``.

    ``voxel_size``: when given, both clouds go through ``preprocess.voxel_down_sample(cloud, voxel_size)`` first, and
    descriptors, matching and the pose search run on the down-sampled clouds (FPFH stops being discriminative on dense
    clouds).  ``fitness`` and ``inliers`` of the result then refer to the down-sampled clouds and their correspondences, not
    to the rows of ``source`` and ``target``; the pose holds for the full clouds all the same."""
    if method not in ("ransac", "fgr"):
        raise ValueError("method must be 'ransac' or 'fgr', got %r" % (method,))
    src, tgt = _as_rows(source, "source", 3), _as_rows(target, "target", 3)
    _check_tau(max_distance)
    _single_process("registration_global")
    device = kwargs.get("device")
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
    if method == "fgr":
        return GlobalResult(*registration_fgr(src, tgt, pairs, max_distance=max_distance, **kwargs)[:4])
    return registration_ransac(src, tgt, pairs, max_distance, **kwargs)
