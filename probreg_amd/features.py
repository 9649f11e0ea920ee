"""Feature generators of the L2-distance registrations - drop-in for ``probreg.features`` (reference
probreg/features.py:11-69): ``Feature`` and ``GMM``.

The reference's ``GMM.compute`` fits ``sklearn.mixture.GaussianMixture(n_components, covariance_type="spherical")`` to
the cloud before every optimisation; that fit dominates GMMReg.  Here it runs in ``libprobreg_hip.so``
(``prg_gmmfit_*``, csrc/gmmfit.hip) in fp64: greedy k-means++ seeding, Lloyd iterations to convergence, the M-step on
the one-hot labels that scikit-learn starts from, then EM with scikit-learn's formulas and stop test.  scikit-learn is
not imported.

Differences a caller can see (on purpose):
  * ``random_state`` defaults to 0, so two calls give byte-identical mixtures (every sum over points runs in a fixed
    order); the reference leaves scikit-learn unseeded.  The uniforms of the D^2 sampling are drawn on the host from
    ``numpy.random.RandomState(random_state)``; everything else of the initialisation runs on the device.  The seeds
    differ from scikit-learn's for the same ``random_state`` (other consumption of the stream), the quality does not
    (DESIGN.md).
  * ``weights_init``, ``means_init`` and ``precisions_init`` are given together or not at all; given, EM starts from
    them and reproduces scikit-learn's result to rounding.
  * Clouds of dimension 2 or 3.  The reference's other two generators are provided in modules of their own and not
    under this module's name: ``FPFH`` in ``probreg_amd.fpfh``, ``OneClassSVM`` in ``probreg_amd.svm``.
"""
import abc
import ctypes

import numpy as np

from . import _lib

MAX_SEED_TRIALS = 16
LLOYD_MAX_ITER = 300  # sklearn.cluster.KMeans defaults
LLOYD_TOL = 1.0e-4


class Feature(abc.ABC):
    @abc.abstractmethod
    def init(self):
        pass

    @abc.abstractmethod
    def compute(self, data):
        return None

    def annealing(self):
        pass

    def __call__(self, data):
        return self.compute(data)


class GmmFitPlan(_lib.Handle):
    """One ``prg_gmmfit`` handle: a cloud on one device / stream and the stages of the fit."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_gmmfit_create, _lib.lib.prg_gmmfit_destroy, device)
        self.n = 0
        self.dim = 0
        self.k = 0

    def set_data(self, data):
        data = np.ascontiguousarray(data, dtype=np.float64)
        _lib.check(_lib.lib.prg_gmmfit_set_data(self._h, _lib.ptr(data), data.shape[0], data.shape[1]))
        self.n, self.dim = data.shape

    def seed(self, k, uniforms):
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        _lib.check(_lib.lib.prg_gmmfit_seed(self._h, int(k), _lib.ptr(uniforms), uniforms.shape[1]))
        self.k = int(k)

    def seeds(self):
        idx = np.empty(self.k, dtype=np.int32)
        _lib.check(_lib.lib.prg_gmmfit_get_seeds(self._h, _lib.ptr(idx)))
        return idx

    def lloyd(self, max_iter, tol):
        it = ctypes.c_int(0)
        _lib.check(_lib.lib.prg_gmmfit_lloyd(self._h, int(max_iter), float(tol), ctypes.byref(it)))
        return int(it.value)

    def init_from_labels(self, reg_covar):
        _lib.check(_lib.lib.prg_gmmfit_init_from_labels(self._h, float(reg_covar)))

    def set_params(self, weights, means, precisions):
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        means = np.ascontiguousarray(means, dtype=np.float64)
        precisions = np.ascontiguousarray(precisions, dtype=np.float64)
        k = weights.shape[0]
        if weights.ndim != 1 or means.shape != (k, self.dim) or precisions.shape != (k,):
            raise ValueError("weights (k,), means (k, %d) and precisions (k,) expected, got %s, %s, %s"
                             % (self.dim, weights.shape, means.shape, precisions.shape))
        _lib.check(_lib.lib.prg_gmmfit_set_params(self._h, k, _lib.ptr(weights), _lib.ptr(means), _lib.ptr(precisions)))
        self.k = k

    def em(self, tol, max_iter, reg_covar):
        """(n_iter, converged, lower bound of every iteration)."""
        it, conv = ctypes.c_int(0), ctypes.c_int(0)
        lbs = np.zeros(int(max_iter))
        _lib.check(_lib.lib.prg_gmmfit_em(self._h, float(tol), int(max_iter), float(reg_covar), ctypes.byref(it),
                                          ctypes.byref(conv), _lib.ptr(lbs)))
        return int(it.value), bool(conv.value), lbs[:it.value].copy()

    def params(self):
        """(weights (k,), means (k, dim), covariances (k,))."""
        w = np.empty(self.k)
        mu = np.empty((self.k, self.dim))
        cov = np.empty(self.k)
        _lib.check(_lib.lib.prg_gmmfit_get_params(self._h, _lib.ptr(w), _lib.ptr(mu), _lib.ptr(cov)))
        return w, mu, cov

    def centers(self):
        mu = np.empty((self.k, self.dim))
        _lib.check(_lib.lib.prg_gmmfit_get_params(self._h, None, _lib.ptr(mu), None))
        return mu


def seed_trials(n_components):
    """Candidates per k-means++ step: 2 + floor(log K), the count scikit-learn uses."""
    return min(2 + int(np.log(n_components)), MAX_SEED_TRIALS)


def seed_uniforms(n_components, random_state):
    """The (K, trials) uniforms of the D^2 sampling; entry [0, 0] draws the first centre."""
    rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    return rs.random_sample((int(n_components), seed_trials(n_components)))


def lloyd_tolerance(data, tol=LLOYD_TOL):
    """scikit-learn's KMeans turns its relative ``tol`` into mean(var(data, axis=0)) * tol on the summed squared shift."""
    return float(np.mean(np.var(data, axis=0)) * tol)


class GMM(Feature):
    """Feature points of a cloud: the means and weights of a spherical Gaussian mixture (reference features.py:54-69).

    Args:
        n_gmm_components: number of mixture components (K <= number of points, else ``compute`` raises ValueError).
    Extensions (keywords with defaults): ``random_state`` (seed of the initialisation), ``tol`` / ``max_iter`` /
    ``reg_covar`` (scikit-learn's EM stop tolerance 1e-3, iteration cap 100, covariance floor 1e-6),
    ``weights_init`` / ``means_init`` / ``precisions_init`` (explicit start, all three together), ``device``.
    After ``compute``: ``means_``, ``weights_``, ``covariances_``, ``n_iter_``, ``converged_``, ``lower_bound_``
    (of the last iteration), ``lower_bounds_`` (every iteration) as in scikit-learn, and ``n_lloyd_iter_``.
    """

    def __init__(self, n_gmm_components=800, random_state=0, tol=1.0e-3, max_iter=100, reg_covar=1.0e-6,
                 weights_init=None, means_init=None, precisions_init=None, device=None):
        self._n_gmm_components = int(n_gmm_components)
        self._random_state = random_state
        self._tol = tol
        self._max_iter = int(max_iter)
        self._reg_covar = reg_covar
        given = [a is not None for a in (weights_init, means_init, precisions_init)]
        if any(given) and not all(given):
            raise ValueError("weights_init, means_init and precisions_init are given together or not at all")
        self._init = (weights_init, means_init, precisions_init) if all(given) else None
        if self._n_gmm_components < 1:
            raise ValueError("n_gmm_components must be >= 1, got %d" % self._n_gmm_components)
        if self._max_iter < 1:
            raise ValueError("max_iter must be >= 1, got %d" % self._max_iter)
        self._device = device
        self.init()

    def init(self):
        """A fresh estimator (features.py:64-65): forgets the previous fit."""
        self.means_ = self.weights_ = self.covariances_ = None
        self.n_iter_ = self.n_lloyd_iter_ = 0
        self.converged_ = False
        self.lower_bound_ = -np.inf
        self.lower_bounds_ = []

    def compute(self, data):
        """Fit the mixture to ``data`` (n, 2 or 3) and return ``(means_, weights_)`` (features.py:67-69)."""
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[1] not in (2, 3):
            raise ValueError("data must be (n, 2) or (n, 3), got shape %s" % (data.shape,))
        k = self._n_gmm_components
        if data.shape[0] < k:
            raise ValueError("Expected n_samples >= n_components but got n_components = %d, n_samples = %d"
                             % (k, data.shape[0]))
        if not np.all(np.isfinite(data)):
            raise ValueError("data contains NaN or infinity")
        plan = GmmFitPlan(self._device)
        try:
            plan.set_data(data)
            if self._init is not None:
                plan.set_params(*self._init)
                if plan.k != k:
                    raise ValueError("the initial parameters describe %d components, n_gmm_components is %d"
                                     % (plan.k, k))
                self.n_lloyd_iter_ = 0
            else:
                plan.seed(k, seed_uniforms(k, self._random_state))
                self.n_lloyd_iter_ = plan.lloyd(LLOYD_MAX_ITER, lloyd_tolerance(data))
                plan.init_from_labels(self._reg_covar)
            self.n_iter_, self.converged_, lbs = plan.em(self._tol, self._max_iter, self._reg_covar)
            self.weights_, self.means_, self.covariances_ = plan.params()
        finally:
            plan.close()
        self.lower_bounds_ = list(lbs)
        self.lower_bound_ = float(lbs[-1])
        return self.means_, self.weights_
