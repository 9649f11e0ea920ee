"""Cost functions of the L2-distance registrations on the GPU (reference probreg/cost_functions.py:15-102).

``compute_l2_dist`` is the Gauss-transform-bound kernel every BFGS evaluation calls; the reference evaluates it through
IFGT for wide kernels, here it is always the direct sum over all pairs.  ``RigidCostFunction`` and
``TPSCostFunction`` are the objectives of GMMReg (``l2dist_regs``): small host algebra around that kernel, operating on
the K-component mixtures that ``features.GMM`` extracts, not on the clouds.
"""
import abc

import numpy as np

from . import gauss_transform as gt
from . import se3_op as so
from . import transformation as tf


class CostFunction(abc.ABC):
    """An objective of ``scipy.optimize.minimize(jac=True)``: ``theta -> (value, gradient)`` (cost_functions.py:15-30)."""

    def __init__(self, tf_type):
        self._tf_type = tf_type

    @abc.abstractmethod
    def to_transformation(self, theta):
        return None

    @abc.abstractmethod
    def initial(self):
        return None

    @abc.abstractmethod
    def __call__(self, theta, *args):
        return None, None


def compute_l2_dist(mu_source, phi_source, mu_target, phi_target, sigma, exact=False):
    """Returns (-sum_ij phi_s_i phi_t_j N(mu_s_i - mu_t_j; 2 sigma^2), gradient w.r.t. mu_source).

    ``exact`` (an extension): exponentials in fp64 instead of fp32, the reference's own precision.  The cost functions
    below use it: they see K x K component pairs, and BFGS amplifies the 1e-7 per term of the fp32 exponential."""
    mu_source = np.asarray(mu_source, dtype=np.float64)
    mu_target = np.asarray(mu_target, dtype=np.float64)
    phi_source = np.asarray(phi_source, dtype=np.float64)
    phi_target = np.asarray(phi_target, dtype=np.float64)
    z = np.power(2.0 * np.pi * sigma ** 2, mu_source.shape[1] * 0.5)
    gtrans = gt.GaussTransform(mu_target, np.sqrt(2.0) * sigma, exact=exact)
    # one launch group for the scalar weights and the D coordinate-weighted rows (cost_functions.py:38-39)
    weights = np.concatenate([(phi_target / z)[None, :], phi_target * mu_target.T / z], axis=0)
    res = gtrans.compute(mu_source, weights)
    phi_j_e = res[0]
    phi_mu_j_e = res[1:].T
    g = (phi_source * phi_j_e * mu_source.T - phi_source * phi_mu_j_e.T).T / (2.0 * sigma ** 2)
    return -np.dot(phi_source, phi_j_e), g


class RigidCostFunction(CostFunction):
    """L2 distance under a rigid motion; ``theta = (quaternion w x y z, translation)`` (cost_functions.py:44-65).

    The gradient by the quaternion goes through ``se3_op.diff_rot_from_quaternion``.  By default in the reference's
    form, which is not the derivative away from the identity (see there): BFGS then follows the reference's path and
    stops where the reference stops.  ``exact_gradient=True`` (an extension) uses the derivative."""

    def __init__(self, exact_gradient=False):
        super(RigidCostFunction, self).__init__(tf.RigidTransformation)
        self._exact_gradient = bool(exact_gradient)

    def to_transformation(self, theta):
        return self._tf_type(so.quat2mat(theta[:4]), theta[4:7])

    def initial(self):
        x0 = np.zeros(7)
        x0[0] = 1.0
        return x0

    def __call__(self, theta, *args):
        mu_source, phi_source, mu_target, phi_target, sigma = args
        moved = self.to_transformation(theta).transform(mu_source)
        f, g = compute_l2_dist(moved, phi_source, mu_target, phi_target, sigma, exact=True)
        # chain rule: d f / d q_i = <g^T mu_source, dR / d q_i>, d f / d t = column sums of g
        d_rot = so.diff_rot_from_quaternion(theta[:4], reference_form=not self._exact_gradient)
        grad_q = np.einsum("ab,iab->i", np.dot(g.T, mu_source), d_rot)
        return f, np.concatenate([grad_q, g.sum(axis=0)])


class TPSCostFunction(CostFunction):
    """L2 distance under a thin-plate spline on ``control_pts`` plus ``beta`` times its bending energy;
    ``theta`` = the affine part (dim + 1, dim) then the warp coefficients (K - dim - 1, dim), flattened
    (cost_functions.py:68-102)."""

    def __init__(self, control_pts, alpha=1.0, beta=0.1):
        super(TPSCostFunction, self).__init__(tf.TPSTransformation)
        self._alpha = alpha
        self._beta = beta
        self._control_pts = control_pts

    def to_transformation(self, theta):
        dim = self._control_pts.shape[1]
        n_affine = dim * (dim + 1)
        return self._tf_type(theta[:n_affine].reshape(dim + 1, dim), theta[n_affine:].reshape(-1, dim),
                             self._control_pts)

    def initial(self):
        n, dim = self._control_pts.shape
        theta = np.zeros((n, dim))
        theta[1:dim + 1] = np.identity(dim)
        return theta.ravel()

    def __call__(self, theta, *args):
        mu_source, phi_source, mu_target, phi_target, sigma = args
        dim = self._control_pts.shape[1]
        tf_obj = self.to_transformation(theta)
        basis, kernel = tf_obj.prepare(mu_source)
        moved = tf_obj.transform_basis(basis)
        kv = np.dot(kernel, tf_obj.v)
        bending = np.sum(tf_obj.v * kv)  # trace(v^T K v)
        f_self, g_self = compute_l2_dist(moved, phi_source, moved, phi_source, sigma, exact=True)
        f_cross, g_cross = compute_l2_dist(moved, phi_source, mu_target, phi_target, sigma, exact=True)
        f = 2.0 * f_cross - f_self
        g = 2.0 * g_cross - 2.0 * g_self
        grad = self._alpha * np.dot(basis.T, g)
        grad[dim + 1:] += 2.0 * self._beta * kv
        return self._alpha * f + self._beta * bending, grad.ravel()
