"""``FPFH``: Fast Point Feature Histograms - drop-in for ``probreg.features.FPFH`` (reference probreg/features.py:28-51),
which lives here and not in ``probreg_amd.features``.

The reference gets the descriptor from Open3D (``estimate_normals`` with a hybrid search, ``compute_fpfh_feature``).  Here
it runs in ``libprobreg_hip.so`` (``prg_fpfh_*``, csrc/fpfh.hip) in fp64: a uniform-grid neighbour search, PCA normals,
the simplified point feature histograms and their 1 / d^2 weighted gather.  DESIGN.md section 3.9 is the definition,
with the tie rules Open3D leaves to its kd-tree and eigen-solver.  Neither Open3D nor scikit-learn is imported.

Differences a caller can see (on purpose):
  * ``compute`` takes and returns arrays; ``estimate_normals`` accepts an array or anything with ``.points`` and returns
    the normals (the reference's mutates an Open3D cloud: an object with a ``.normals`` attribute gets it set here too).
  * Normals carry no viewpoint orientation (as the reference's for a fresh cloud); their sign is fixed by the rule "the
    component of largest magnitude is positive", so two calls give byte-identical descriptors.
  * ``max_nn_normal`` / ``max_nn_feature`` (Open3D's 30 / 100) are keywords, bounded by ``max_neighbours()``.
  * Clouds of dimension 3.
"""
import ctypes

import numpy as np

from . import _lib
from .features import Feature

N_BINS = 33
SEARCH_NORMALS = 0
SEARCH_FEATURES = 1


def max_neighbours():
    """Longest neighbour list of a search: the upper bound of ``max_nn`` (needs no GPU)."""
    k = ctypes.c_int(0)
    _lib.check(_lib.lib.prg_fpfh_max_nn(ctypes.byref(k)))
    return int(k.value)


class FpfhPlan(_lib.Handle):
    """One ``prg_fpfh`` handle: a cloud on one device / stream and the stages of the descriptor."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_fpfh_create, _lib.lib.prg_fpfh_destroy, device)
        self.n = 0
        self.max_nn = [0, 0]

    def set_data(self, points):
        points = _lib.as_cloud(points, "data", (3,))
        _lib.check(_lib.lib.prg_fpfh_set_data(self._h, _lib.ptr(points), points.shape[0]))
        self.n = points.shape[0]

    def search(self, which, radius, max_nn):
        _lib.check(_lib.lib.prg_fpfh_search(self._h, int(which), float(radius), int(max_nn)))
        self.max_nn[int(which)] = int(max_nn)

    def neighbours(self, which):
        """(idx (n, max_nn) int32 with -1 behind the list, d2 (n, max_nn), count (n,) int32)."""
        k = self.max_nn[int(which)]
        idx = np.empty((self.n, k), dtype=np.int32)
        d2 = np.empty((self.n, k))
        cnt = np.empty(self.n, dtype=np.int32)
        _lib.check(_lib.lib.prg_fpfh_get_neighbours(self._h, int(which), _lib.ptr(idx), _lib.ptr(d2), _lib.ptr(cnt)))
        return idx, d2, cnt

    def compute_normals(self):
        _lib.check(_lib.lib.prg_fpfh_normals(self._h))

    def set_normals(self, normals):
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        if normals.shape != (self.n, 3):
            raise ValueError("normals must be (%d, 3), got shape %s" % (self.n, normals.shape))
        _lib.check(_lib.lib.prg_fpfh_set_normals(self._h, _lib.ptr(normals)))

    def normals(self):
        out = np.empty((self.n, 3))
        _lib.check(_lib.lib.prg_fpfh_get_normals(self._h, _lib.ptr(out)))
        return out

    def compute_spfh(self):
        _lib.check(_lib.lib.prg_fpfh_spfh(self._h))

    def spfh(self):
        out = np.empty((self.n, N_BINS))
        _lib.check(_lib.lib.prg_fpfh_get_spfh(self._h, _lib.ptr(out)))
        return out

    def compute_fpfh(self):
        _lib.check(_lib.lib.prg_fpfh_fpfh(self._h))

    def fpfh(self):
        out = np.empty((self.n, N_BINS))
        _lib.check(_lib.lib.prg_fpfh_get_fpfh(self._h, _lib.ptr(out)))
        return out


class FPFH(Feature):
    """Fast Point Feature Histograms (reference features.py:28-51).

    Args:
        radius_normal: radius of the neighbour search of the normals.
        radius_feature: radius of the neighbour search of the histograms.
    Extensions (keywords with defaults): ``max_nn_normal`` / ``max_nn_feature`` (the 30 / 100 the reference hands to
    Open3D's hybrid search; 1 <= max_nn <= ``max_neighbours()``), ``device``.
    After ``compute``: ``normals_`` (n, 3).
    """

    def __init__(self, radius_normal=0.1, radius_feature=0.5, max_nn_normal=30, max_nn_feature=100, device=None):
        self._radius_normal = radius_normal
        self._radius_feature = radius_feature
        self._max_nn_normal = max_nn_normal
        self._max_nn_feature = max_nn_feature
        self._device = device
        self._check_params()
        self.init()

    def _check_params(self):
        for name, r in (("radius_normal", self._radius_normal), ("radius_feature", self._radius_feature)):
            if not (np.isfinite(r) and r > 0.0):
                raise ValueError("%s must be > 0 and finite, got %r" % (name, r))
        bound = max_neighbours()
        for name, k in (("max_nn_normal", self._max_nn_normal), ("max_nn_feature", self._max_nn_feature)):
            if int(k) != k or not 1 <= k <= bound:
                raise ValueError("%s must be an integer in 1 .. %d, got %r" % (name, bound, k))

    def init(self):
        """Nothing to reset in the reference (features.py:40-41); here the normals of the last ``compute`` go."""
        self.normals_ = None

    def _normals_on(self, plan):
        plan.search(SEARCH_NORMALS, self._radius_normal, self._max_nn_normal)
        plan.compute_normals()
        return plan.normals()

    def estimate_normals(self, data):
        """Unit normals (n, 3) of an (n, 3) array or of an object with ``.points`` (features.py:43-44); an object that
        has a ``.normals`` attribute gets them assigned as well."""
        self._check_params()
        pts = _lib.as_cloud(data, "data", (3,))
        plan = FpfhPlan(self._device)
        try:
            plan.set_data(pts)
            normals = self._normals_on(plan)
        finally:
            plan.close()
        if hasattr(data, "normals") and not isinstance(data, np.ndarray):
            data.normals = normals
        return normals

    def compute(self, data):
        """The (n, 33) float64 descriptors of ``data`` (n, 3) (features.py:46-51)."""
        self._check_params()
        pts = _lib.as_cloud(data, "data", (3,))
        plan = FpfhPlan(self._device)
        try:
            plan.set_data(pts)
            self.normals_ = self._normals_on(plan)
            plan.search(SEARCH_FEATURES, self._radius_feature, self._max_nn_feature)
            plan.compute_spfh()
            plan.compute_fpfh()
            return plan.fpfh()
        finally:
            plan.close()
