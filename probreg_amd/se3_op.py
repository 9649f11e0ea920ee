"""Quaternion helpers of the rigid L2-distance cost (reference probreg/se3_op.py:62-120 and the ``quat2mat`` of
transforms3d that it calls).  Host code: a 3 x 3 matrix and its four derivatives per BFGS evaluation.

The twist helpers of the same reference module (``skew``, ``twist_trans``, ``twist_mul``) live in ``gmmtree``.
"""
import numpy as np

_EPS = np.finfo(np.float64).eps


def quat2mat(q):
    """Rotation matrix of the quaternion ``q = (w, x, y, z)``: R = I + (2 / |q|^2) A(q) with A quadratic in q, so any
    non-zero quaternion is valid (it is normalised implicitly); the identity when |q|^2 is below the float64 epsilon.
    This is the convention of ``transforms3d.quaternions.quat2mat``."""
    w, x, y, z = (float(v) for v in np.asarray(q, dtype=np.float64)[:4])
    nq = w * w + x * x + y * y + z * z
    if nq < _EPS:
        return np.identity(3)
    return np.identity(3) + (2.0 / nq) * _quad(w, x, y, z)


def _quad(w, x, y, z):
    return np.array([[-(y * y + z * z), x * y - w * z, x * z + w * y],
                     [x * y + w * z, -(x * x + z * z), y * z - w * x],
                     [x * z - w * y, y * z + w * x, -(x * x + y * y)]])


def _dquad(w, x, y, z):
    """dA / d(w, x, y, z): A is quadratic, so each slice is linear in q."""
    return np.array([[[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]],
                     [[0.0, y, z], [y, -2.0 * x, -w], [z, w, -2.0 * x]],
                     [[-2.0 * y, x, w], [x, 0.0, z], [-w, z, -2.0 * y]],
                     [[-2.0 * z, -w, x], [w, -2.0 * z, y], [x, y, 0.0]]])


def diff_rot_from_quaternion(q, reference_form=False):
    """dR(q) / dq as a (4, 3, 3) array, slice i the derivative by q[i] (reference se3_op.py:62-120).

    With n = |q|^2 the chain rule on R = I + (2 / n) A gives  dR/dq_i = (2 / n) dA/dq_i - (2 q_i / n) (R - I),
    which is what this returns by default (it matches central differences of ``quat2mat`` for any q).

    ``reference_form=True`` returns what the reference's function returns instead.  It differs from the derivative in
    two places: the second term of the six off-diagonal entries is divided by n^2 instead of n (equal on unit
    quaternions), and the entries [2, 2, 2] and [3, 2, 2] are -4 q_2 (q_1^2 + q_2^2) / n^2 and 4 q_3 (q_3^2 + q_0^2) / n^2
    where the derivative has -4 q_2 (q_0^2 + q_3^2) / n^2 and 4 q_3 (q_1^2 + q_2^2) / n^2 (equal only where q_2 or q_3
    vanish, e.g. at the identity, where BFGS starts).  ``RigidCostFunction`` uses the reference's form by default so
    that an optimisation follows the reference step by step; its ``exact_gradient=True`` uses the derivative."""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = (float(v) for v in q[:4])
    n = w * w + x * x + y * y + z * z
    off = quat2mat(q) - np.identity(3)
    first = (2.0 / n) * _dquad(w, x, y, z)
    if not reference_form:
        return first - (2.0 / n) * q[:4, None, None] * off[None]
    second = np.where(np.identity(3, dtype=bool), off / n, off / (n * n))
    d = first - 2.0 * q[:4, None, None] * second[None]
    d[2, 2, 2] = -4.0 * y * (x * x + y * y) / (n * n)
    d[3, 2, 2] = 4.0 * z * (z * z + w * w) / (n * n)
    return d
