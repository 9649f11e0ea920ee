"""``OneClassSVM``: the feature generator of support-vector registration - drop-in for ``probreg.features.OneClassSVM``
(reference probreg/features.py:72-100), which lives here and not in ``probreg_amd.features``.

The reference's ``compute`` fits ``sklearn.svm.OneClassSVM(nu, kernel="rbf", gamma)`` (libsvm) to the cloud before every
optimisation; that fit is the cost of SVR that grows with the cloud.  Here it runs in ``libprobreg_hip.so``
(``prg_ocsvm_*``, csrc/ocsvm.hip) in fp64: the same dual in libsvm's scaling, libsvm's start, pair choice (WSS2), stop test
(maximal KKT violation < ``tol``) and ``rho``, solved by working-set decomposition.  scikit-learn is not imported.

Differences a caller can see (on purpose):
  * The solution satisfies the same stop test as libsvm's, it is not the same vector: two ``tol``-optimal points of an
    ill-conditioned problem differ in single coefficients and in the support set, while objective and decision function
    agree within what ``tol`` determines.  Two calls here give byte-identical results.
  * ``max_iter`` counts rounds of the decomposition (working sets), not single SMO steps, and ``n_iter_`` reports rounds;
    ``n_inner_iter_`` is the number of SMO steps.  When ``max_iter`` ends the solve, ``converged_`` is False and the
    current (feasible) solution is returned, as with libsvm's warning.
  * Clouds of dimension 2 or 3.
"""
import ctypes

import numpy as np

from . import _lib
from .features import Feature
from .log import log

DEFAULT_MAX_ITER = 100000


def working_set_size():
    """Points per working set of the solver (needs no GPU)."""
    q = ctypes.c_int(0)
    _lib.check(_lib.lib.prg_ocsvm_working_set_size(ctypes.byref(q)))
    return int(q.value)


class OcsvmPlan(_lib.Handle):
    """One ``prg_ocsvm`` handle: a cloud on one device / stream, its solve and the solution."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_ocsvm_create, _lib.lib.prg_ocsvm_destroy, device)
        self.n = 0
        self.dim = 0

    def set_data(self, data):
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2:
            raise ValueError("data must be (n, 2) or (n, 3), got shape %s" % (data.shape,))
        _lib.check(_lib.lib.prg_ocsvm_set_data(self._h, _lib.ptr(data), data.shape[0], data.shape[1]))
        self.n, self.dim = data.shape

    def set_profile(self, on):
        _lib.check(_lib.lib.prg_ocsvm_set_profile(self._h, int(bool(on))))

    def profile(self):
        """Device milliseconds of the last solve: (initial gradient, selection, subproblem, gradient sweep)."""
        ms = np.zeros(4)
        _lib.check(_lib.lib.prg_ocsvm_get_profile(self._h, _lib.ptr(ms)))
        return ms

    def solve(self, gamma, nu, tol=1.0e-3, max_iter=DEFAULT_MAX_ITER, inner_cap=None):
        """(rounds, SMO steps, converged, gap)."""
        if inner_cap is None:
            inner_cap = 4 * working_set_size()
        it, inner, conv, gap = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_double(0.0)
        _lib.check(_lib.lib.prg_ocsvm_solve(self._h, float(gamma), float(nu), float(tol), int(max_iter), int(inner_cap),
                                            ctypes.byref(it), ctypes.byref(inner), ctypes.byref(conv),
                                            ctypes.byref(gap)))
        return int(it.value), int(inner.value), bool(conv.value), float(gap.value)

    def solution(self):
        """(alpha (n,), rho, objective, support (n_SV,) int32 ascending)."""
        alpha = np.empty(self.n)
        rho, obj, nsv = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_int(0)
        _lib.check(_lib.lib.prg_ocsvm_get_solution(self._h, _lib.ptr(alpha), ctypes.byref(rho), ctypes.byref(obj),
                                                   ctypes.byref(nsv)))
        support = np.empty(int(nsv.value), dtype=np.int32)
        _lib.check(_lib.lib.prg_ocsvm_get_support(self._h, _lib.ptr(support)))
        return alpha, float(rho.value), float(obj.value), support

    def decision(self, points):
        """sum_i alpha_i k(x_i, p) at ``points`` (k, dim)."""
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != self.dim:
            raise ValueError("points must be (k, %d), got shape %s" % (self.dim, points.shape))
        out = np.empty(points.shape[0])
        _lib.check(_lib.lib.prg_ocsvm_decision(self._h, _lib.ptr(points), points.shape[0], _lib.ptr(out)))
        return out


class OneClassSVM(Feature):
    """Feature points of a cloud: the support vectors and dual coefficients of a one-class SVM (reference
    features.py:72-100).

    Args:
        dim: dimension of the samples.
        sigma: scale of the Gaussians the SVM's coefficients are turned into weights of.
        gamma: coefficient of the RBF kernel.
        nu: upper bound on the fraction of training errors, lower bound on the fraction of support vectors.
        delta: annealing factor of ``gamma``.
    Extensions (keywords with defaults): ``tol`` (scikit-learn's stop tolerance 1e-3), ``max_iter`` (rounds of the
    decomposition), ``device``.
    After ``compute``: ``support_``, ``support_vectors_``, ``dual_coef_`` (1, n_SV), ``offset_`` as in scikit-learn,
    ``n_iter_`` (rounds), ``n_inner_iter_`` (SMO steps), ``converged_``, ``gap_`` and ``decision_function(points)``.
    """

    def __init__(self, dim, sigma, gamma=0.5, nu=0.05, delta=10.0, tol=1.0e-3, max_iter=DEFAULT_MAX_ITER, device=None):
        self._dim = dim
        self._sigma = sigma
        self._gamma = gamma
        self._nu = nu
        self._delta = delta
        self._tol = tol
        self._max_iter = int(max_iter)
        self._device = device
        self._plan = None
        self.init()

    def init(self):
        """A fresh estimator (features.py:91-92): forgets the previous fit."""
        if getattr(self, "_plan", None) is not None:
            self._plan.close()
        self._plan = None
        self.support_ = self.support_vectors_ = self.dual_coef_ = None
        self.offset_ = None
        self.n_iter_ = self.n_inner_iter_ = 0
        self.converged_ = False
        self.gap_ = np.inf

    def compute(self, data):
        """Fit the SVM to ``data`` (n, 2 or 3) and return ``(support_vectors_, dual_coef_[0] * (2 pi sigma^2)^(dim/2))``
        (features.py:94-97)."""
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[1] not in (2, 3):
            raise ValueError("data must be (n, 2) or (n, 3), got shape %s" % (data.shape,))
        if self._plan is not None:
            self._plan.close()
        self._plan = plan = OcsvmPlan(self._device)
        plan.set_data(data)
        self.n_iter_, self.n_inner_iter_, self.converged_, self.gap_ = plan.solve(self._gamma, self._nu, self._tol,
                                                                                   self._max_iter)
        if not self.converged_:  # libsvm's "reaching max number of iterations" / scikit-learn's ConvergenceWarning
            log.warning("OneClassSVM: the solve ended at max_iter = %d rounds with a KKT violation of %.3e (tol %.3e); "
                        "the returned solution is feasible but not optimal", self._max_iter, self.gap_, self._tol)
        alpha, rho, _, support = plan.solution()
        self.support_ = support
        self.support_vectors_ = data[support]
        self.dual_coef_ = alpha[support][None, :]
        self.offset_ = np.array([rho])
        z = np.power(2.0 * np.pi * self._sigma ** 2, self._dim * 0.5)
        return self.support_vectors_, self.dual_coef_[0] * z

    def decision_function(self, points):
        """scikit-learn's sign convention: sum_i alpha_i k(x_i, p) - rho, for the last ``compute``."""
        if self._plan is None:
            raise ValueError("decision_function needs a fitted estimator: call compute first")
        return self._plan.decision(points) - self.offset_[0]

    def annealing(self):
        self._gamma *= self._delta
