"""GMMReg and SVR: registration by the L2 distance between Gaussian mixtures - drop-in for ``probreg.l2dist_regs``
(reference probreg/l2dist_regs.py; Jian & Vemuri, "Robust Point Set Registration Using Gaussian Mixture Models", PAMI
2011; Campbell & Petersson, "An Adaptive Data Representation for Robust Point-Set Registration and Merging", ICCV 2015).

What runs where
  * The mixture fit of both clouds (``features.GMM``; the reference calls scikit-learn, and that fit dominates): HIP,
    ``prg_gmmfit_*``.
  * The one-class SVM fit of both clouds (``svm.OneClassSVM``; the reference calls scikit-learn / libsvm): HIP,
    ``prg_ocsvm_*``.
  * Every BFGS evaluation's Gauss transforms over the K x K component pairs (``cost_functions.compute_l2_dist``): HIP.
  * The optimiser itself, ``scipy.optimize.minimize(method="BFGS", jac=True)`` on 7 (rigid) or K * dim (thin-plate
    spline) unknowns, and the small algebra of the cost functions: host, as in the reference.

``L2DistRegistration`` is generic in its feature generator and cost function: GMMReg (``RigidGMMReg``, ``TPSGMMReg``,
``registration_gmmreg``) feeds it mixture centres and weights, SVR (``RigidSVR``, ``TPSSVR``, ``registration_svr``) the
support vectors and scaled dual coefficients of a one-class SVM.  The SVM feature generator is ``probreg_amd.svm.OneClassSVM``
(the reference keeps it in ``features``).
"""
import logging

import numpy as np
from scipy.optimize import minimize

from . import cost_functions as cf
from . import features as ft
from ._lib import as_points as _as_points
from .svm import OneClassSVM
from .log import log


class L2DistRegistration(object):
    """L2 distance registration (reference l2dist_regs.py:16-97).

    Args:
        source: source cloud (n, dim).
        feature_gen (features.Feature): turns a cloud into mixture centres and weights.
        cost_fn (cost_functions.CostFunction): the L2 distance as a function of the transformation parameters.
        sigma: scale of the L2 distance.
        delta: annealing factor of ``sigma`` per outer iteration.
        use_estimated_sigma: estimate ``sigma`` from the source cloud.
    """

    def __init__(self, source, feature_gen, cost_fn, sigma=1.0, delta=0.9, use_estimated_sigma=True):
        self._source = source
        self._feature_gen = feature_gen
        self._cost_fn = cost_fn
        self._sigma = sigma
        self._delta = delta
        self._use_estimated_sigma = use_estimated_sigma
        self._callbacks = []
        if self._source is not None and self._use_estimated_sigma:
            self._estimate_sigma(self._source)

    def set_source(self, source):
        self._source = source
        if self._use_estimated_sigma:
            self._estimate_sigma(self._source)

    def set_callbacks(self, callbacks):
        self._callbacks.extend(callbacks)

    def _estimate_sigma(self, data):
        # det(sample covariance)^(1 / (2 dim)): the geometric mean of the cloud's principal standard deviations
        ndata, dim = data.shape
        centred = data - np.mean(data, axis=0)
        cov = np.dot(centred.T, centred) / (ndata - 1)
        self._sigma = np.power(np.linalg.det(cov), 1.0 / (2.0 * dim))

    def _annealing(self):
        self._sigma *= self._delta

    def optimization_cb(self, x):
        tf_result = self._cost_fn.to_transformation(x)
        for c in self._callbacks:
            c(tf_result)

    def registration(self, target, maxiter=1, tol=1.0e-3, opt_maxiter=50, opt_tol=1.0e-3):
        """``maxiter`` rounds of (fit both mixtures, BFGS on the cost, anneal sigma); stops early when the cost changes
        by less than ``tol`` between rounds (l2dist_regs.py:71-97)."""
        if maxiter < 1:
            raise ValueError("maxiter must be >= 1, got %r" % (maxiter,))
        f_prev = None
        x = self._cost_fn.initial()
        for _ in range(maxiter):
            self._feature_gen.init()
            mu_source, phi_source = self._feature_gen.compute(self._source)
            mu_target, phi_target = self._feature_gen.compute(target)
            res = minimize(self._cost_fn, x, args=(mu_source, phi_source, mu_target, phi_target, self._sigma),
                           method="BFGS", jac=True, tol=opt_tol,
                           options={"maxiter": opt_maxiter, "disp": log.level == logging.DEBUG},
                           callback=self.optimization_cb)
            self._annealing()
            self._feature_gen.annealing()
            x = res.x
            if f_prev is not None and abs(res.fun - f_prev) < tol:
                break
            f_prev = res.fun
        return self._cost_fn.to_transformation(x)


def _n_components(source, n_gmm_components):
    return min(n_gmm_components, int(source.shape[0] * 0.8))


class RigidGMMReg(L2DistRegistration):
    """GMMReg with a rigid motion (l2dist_regs.py:100-105).  Extensions: ``gmm_params`` (extra keywords of
    ``features.GMM``) and ``exact_gradient`` (see ``cost_functions.RigidCostFunction``; default: the reference's)."""

    def __init__(self, source, sigma=1.0, delta=0.9, n_gmm_components=800, use_estimated_sigma=True, gmm_params={},
                 exact_gradient=False):
        gmm = ft.GMM(_n_components(source, n_gmm_components), **gmm_params)
        super(RigidGMMReg, self).__init__(source, gmm, cf.RigidCostFunction(exact_gradient), sigma, delta,
                                          use_estimated_sigma)


class TPSGMMReg(L2DistRegistration):
    """GMMReg with a thin-plate spline whose control points are the source's mixture centres
    (l2dist_regs.py:108-118).  ``gmm_params``: extra keywords of ``features.GMM``."""

    def __init__(self, source, sigma=1.0, delta=0.9, n_gmm_components=800, alpha=1.0, beta=0.1,
                 use_estimated_sigma=True, gmm_params={}):
        gmm = ft.GMM(_n_components(source, n_gmm_components), **gmm_params)
        super(TPSGMMReg, self).__init__(source, gmm, cf.TPSCostFunction([], alpha, beta), sigma, delta,
                                        use_estimated_sigma)
        self._feature_gen.init()
        control_pts, _ = self._feature_gen.compute(source)
        self._cost_fn._control_pts = control_pts


class RigidSVR(L2DistRegistration):
    """Support-vector registration with a rigid motion (l2dist_regs.py:121-135).  ``_estimate_sigma`` also hands the
    estimated scale to the feature generator (its ``_sigma``, and ``_gamma = 1 / (2 sigma^2)``); the annealing of the
    driver's ``sigma`` does not reach it.  Extension: ``svm_params`` (extra keywords of ``svm.OneClassSVM``)."""

    def __init__(self, source, sigma=1.0, delta=0.9, gamma=0.5, nu=0.1, use_estimated_sigma=True, svm_params={}):
        super(RigidSVR, self).__init__(source, OneClassSVM(source.shape[1], sigma, gamma, nu, **svm_params),
                                       cf.RigidCostFunction(), sigma, delta, use_estimated_sigma)

    def _estimate_sigma(self, data):
        super(RigidSVR, self)._estimate_sigma(data)
        self._feature_gen._sigma = self._sigma
        self._feature_gen._gamma = 1.0 / (2.0 * np.square(self._sigma))


class TPSSVR(L2DistRegistration):
    """Support-vector registration with a thin-plate spline whose control points are the source's support vectors
    (l2dist_regs.py:138-155).  ``svm_params``: extra keywords of ``svm.OneClassSVM``."""

    def __init__(self, source, sigma=1.0, delta=0.9, gamma=0.5, nu=0.1, alpha=1.0, beta=0.1, use_estimated_sigma=True,
                 svm_params={}):
        super(TPSSVR, self).__init__(source, OneClassSVM(source.shape[1], sigma, gamma, nu, **svm_params),
                                     cf.TPSCostFunction([], alpha, beta), sigma, delta, use_estimated_sigma)
        self._feature_gen.init()
        control_pts, _ = self._feature_gen.compute(source)
        self._cost_fn._control_pts = control_pts

    def _estimate_sigma(self, data):
        super(TPSSVR, self)._estimate_sigma(data)
        self._feature_gen._sigma = self._sigma
        self._feature_gen._gamma = 1.0 / (2.0 * np.square(self._sigma))


def registration_gmmreg(source, target, tf_type_name="rigid", callbacks=[], **kargs):
    """GMMReg with the reference's signature (l2dist_regs.py:158-181).

    source, target : (n, dim) arrays or anything with ``.points`` (Open3D point clouds)
    tf_type_name   : 'rigid' or 'nonrigid' (thin-plate spline)
    callbacks      : called after each BFGS iteration with the current transformation
    **kargs        : keywords of :class:`RigidGMMReg` / :class:`TPSGMMReg`
    Returns the transformation from source to target.
    """
    if tf_type_name == "rigid":
        gmmreg = RigidGMMReg(_as_points(source), **kargs)
    elif tf_type_name == "nonrigid":
        gmmreg = TPSGMMReg(_as_points(source), **kargs)
    else:
        raise ValueError("Unknown transform type %s" % tf_type_name)
    gmmreg.set_callbacks(callbacks)
    return gmmreg.registration(_as_points(target))


def registration_svr(source, target, tf_type_name="rigid", maxiter=1, tol=1.0e-3, opt_maxiter=50, opt_tol=1.0e-3,
                     callbacks=[], **kwargs):
    """Support-vector registration with the reference's signature (l2dist_regs.py:184-219).

    source, target : (n, dim) arrays or anything with ``.points`` (Open3D point clouds)
    tf_type_name   : 'rigid' or 'nonrigid' (thin-plate spline)
    maxiter, tol   : rounds of the outer loop and its stop tolerance on the cost
    opt_maxiter, opt_tol : BFGS iterations per round and their tolerance
    callbacks      : called after each BFGS iteration with the current transformation
    **kwargs       : keywords of :class:`RigidSVR` / :class:`TPSSVR`
    Returns the transformation from source to target.
    """
    if tf_type_name == "rigid":
        svr = RigidSVR(_as_points(source), **kwargs)
    elif tf_type_name == "nonrigid":
        svr = TPSSVR(_as_points(source), **kwargs)
    else:
        raise ValueError("Unknown transform type %s" % tf_type_name)
    svr.set_callbacks(callbacks)
    return svr.registration(_as_points(target), maxiter, tol, opt_maxiter, opt_tol)
