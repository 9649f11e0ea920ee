"""Transformation result types of the registration API (reference probreg/transformation.py:17-160).

These are small host-side value objects (a 3x3 matrix, a vector, an M x D weight matrix); the
per-iteration transform of the *source cloud* inside the EM loop runs fused on the GPU
(``k_transform_linear`` / ``k_gw`` in csrc/), not through these classes.
``transform`` keeps the reference's contract (a non-rigid result moves the control points it was fitted on); ``warp`` moves any
points: the non-rigid classes evaluate their continuous displacement field on the GPU (``probreg_amd.field``).
``DeformableKinematicModel`` (transformation.py:163-212) skins its points on the GPU (``prg_dq_skin``).
"""
import abc
import itertools

import numpy as np


def _is_vector3d(points):
    # open3d is optional: duck-type o3.utility.Vector3dVector (reference transformation.py:23-26)
    return type(points).__name__ == "Vector3dVector"


class Transformation(abc.ABC):
    def __init__(self, xp=np):
        self.xp = xp

    def transform(self, points, array_type=None):
        if _is_vector3d(points) or (array_type is not None and isinstance(points, array_type)):
            return type(points)(self._transform(np.asarray(points)))
        return self._transform(points)

    @abc.abstractmethod
    def _transform(self, points):
        return points

    def warp(self, points):
        """Move any points.  For a transformation that is a function of the point alone (rigid, affine, the kinematic model)
        this is ``transform``; the non-rigid results override it with their continuous displacement field."""
        return self.transform(points)


def _field(obj, control, weights, kernel, param=None, device=None):
    """The ``field.KernelField`` a transformation object keeps between ``warp`` calls, holding the control points and weights
    given: created on the first call, set again on every later one (an EM callback sees new weights every iteration),
    released by ``_close_field``."""
    from .field import KernelField

    field = obj.__dict__.get("_warp_field")
    if field is None:
        field = obj.__dict__["_warp_field"] = KernelField(control, weights, kernel, param, device)
    else:
        field.set_control(control, weights, kernel, param)
    return field


def _close_field(obj):
    field = obj.__dict__.pop("_warp_field", None)
    if field is not None:
        field.close()


def _warp_points(points, dim):
    """The points of a ``warp`` call as a finite float64 (n, dim) array (ValueError otherwise); n = 0 is fine."""
    from . import _lib

    return _lib.as_cloud(points, "points", (dim,), min_points=0)


class RigidTransformation(Transformation):
    """x -> scale * rot @ x + t   (reference transformation.py:33-60)."""

    def __init__(self, rot=np.identity(3), t=np.zeros(3), scale=1.0, xp=np):
        super(RigidTransformation, self).__init__(xp)
        self.rot = rot
        self.t = t
        self.scale = scale

    def _transform(self, points):
        return self.scale * np.dot(points, self.rot.T) + self.t

    def inverse(self):
        return RigidTransformation(self.rot.T, -np.dot(self.rot.T, self.t) / self.scale, 1.0 / self.scale)

    def __mul__(self, other):
        return RigidTransformation(
            np.dot(self.rot, other.rot), self.t + self.scale * np.dot(self.rot, other.t), self.scale * other.scale
        )


class AffineTransformation(Transformation):
    """x -> b @ x + t   (reference transformation.py:63-78)."""

    def __init__(self, b=np.identity(3), t=np.zeros(3), xp=np):
        super(AffineTransformation, self).__init__(xp)
        self.b = b
        self.t = t

    def _transform(self, points):
        return np.dot(points, self.b.T) + self.t


class CombinedTransformation(Transformation):
    """x -> scale * rot @ (x + v) + t : non-rigid displacement first, similarity second (reference
    transformation.py:105-121, the result type of BCPD).  ``v`` is one row per point (or 0).

    ``field`` = ``(control, weights, c)``: the continuous displacement ``v(x) = sum_m weights_m / sqrt(|x - control_m|^2 + c)``
    that ``v`` samples at the control points; ``CombinedBCPD`` attaches it, and ``warp`` needs it to move other points."""

    def __init__(self, rot=np.identity(3), t=np.zeros(3), scale=1.0, v=0.0, field=None):
        super(CombinedTransformation, self).__init__()
        self.rigid_trans = RigidTransformation(rot, t, scale)
        self.v = v
        self.field = field

    def _transform(self, points):
        return self.rigid_trans._transform(points + self.v)

    def warp(self, points):
        """``scale * rot @ (x + v(x)) + t`` for any points ``x``, ``v(x)`` evaluated on the GPU in fp64."""
        if self.field is None:
            if np.any(np.asarray(self.v) != 0.0):
                raise ValueError("CombinedTransformation.warp: this object holds its displacement `v` per control point only "
                                 "and no `field=(control, weights, c)` to evaluate it elsewhere (CombinedBCPD attaches one); "
                                 "use transform() on the control points.")
            return self.rigid_trans._transform(np.asarray(points))
        control, weights, c = self.field
        pts = _warp_points(points, np.asarray(control).shape[1])
        return self.rigid_trans._transform(pts + _field(self, control, weights, "imq", c).evaluate(pts))

    def close(self):
        """Release the GPU handle that ``warp`` keeps."""
        _close_field(self)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may be gone already
            pass


class NonRigidTransformation(Transformation):
    """y_m -> y_m + (G W)_m on the control points it was built with (reference transformation.py:81-102).

    ``g`` is the float32 Gaussian kernel matrix of the control points.  When the object comes out
    of ``NonRigidCPD`` the GPU plan holds the kernel as its factor ``G = F F^T`` (or, when the kernel is too narrow to
    factor, as the matrix itself); ``.g`` evaluates / downloads the M x M float32 matrix on first access (M*M*4 bytes).
    """

    def __init__(self, w, points, beta=2.0, xp=np, _plan=None, _plan_points=None, _origin=None):
        super(NonRigidTransformation, self).__init__(xp)
        self._points = np.asarray(points)
        self._beta = beta
        self._plan = _plan
        # the control points as the plan holds them (NonRigidCPD shifts far-from-origin clouds before the float32 upload):
        # _plan_points = points - _origin
        self._plan_points = self._points if _plan_points is None else np.asarray(_plan_points)
        self._origin = np.zeros(self._points.shape[1]) if _origin is None else np.asarray(_origin, dtype=np.float64)
        self._g = None
        self.w = w

    @property
    def g(self):
        if self._g is None:
            if self._plan is not None:
                self._g = self._plan.get_g()
            else:
                from . import math_utils as mu

                self._g = mu.rbf_kernel(self._points, self._points, self._beta)
        return self._g

    def close(self):
        """Release the GPU plan an explicit-array M-step (``NonRigidCPD._maximization_step``) cached on this object, and
        the handle that ``warp`` keeps."""
        cache = self.__dict__.pop("_mstep_plan", None)
        if cache is not None:
            cache[0].close()
        _close_field(self)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may be gone already
            pass

    def _transform(self, points):
        # same contract as the reference: ``points`` must be the control points the kernel was built on
        if self._plan is not None:
            # G W on the GPU (fp64; through the kernel factor, or the float32 G of the dense fallback), never through a host copy of G
            self._plan.set_w(np.asarray(self.w, dtype=np.float64))
            disp = self._plan.nonrigid_apply() - self._plan_points.astype(np.float32).astype(np.float64)
            return np.asarray(points) + disp
        return points + np.dot(self.g, self.w)

    def field_control(self):
        """The control points of the displacement field, in the frame ``x - _origin``: the float32-rounded cloud the kernel
        matrix was built from, as float64."""
        return np.asarray(self._plan_points).astype(np.float32).astype(np.float64)

    def warp(self, points):
        """``x + sum_m exp(-|x - y_m|^2 / (2 beta)) w_m`` for any points ``x``, on the GPU in fp64.  The ``y_m`` are the
        control points as the kernel matrix of ``transform`` saw them; the queries are shifted into their frame in fp64."""
        pts = _warp_points(points, self._points.shape[1])
        w = np.asarray(self.w, dtype=np.float64)
        device = None if self._plan is None else self._plan.device
        return pts + _field(self, self.field_control(), w, "gaussian", self._beta, device).evaluate(pts - self._origin)


def _tps_kernel(x, y):
    from . import math_utils as mu

    return mu.tps_kernel(x, y)


class TPSTransformation(Transformation):
    """Thin-plate spline x -> [1 x] a + U(x, control_pts) N v (reference transformation.py:124-160): ``a`` the affine
    part (dim + 1, dim), ``v`` the warp coefficients (K - dim - 1, dim) in the null space N of [1 control_pts]^T, the
    result type of ``registration_gmmreg(..., "nonrigid")``."""

    def __init__(self, a, v, control_pts, kernel=_tps_kernel):
        super(TPSTransformation, self).__init__()
        self.a = a
        self.v = v
        self.control_pts = control_pts
        self._kernel = kernel

    def prepare(self, landmarks):
        """(basis (m, K), kernel (K - dim - 1, K - dim - 1)): ``basis @ [a; v]`` moves the landmarks and
        ``trace(v^T kernel v)`` is the bending energy."""
        ctrl = self.control_pts
        m, d = landmarks.shape
        n = ctrl.shape[0]
        u, _, _ = np.linalg.svd(np.c_[np.ones((n, 1)), ctrl])
        null = u[:, d + 1:]
        basis = np.c_[np.ones((m, 1)), landmarks, np.dot(self._kernel(landmarks, ctrl), null)]
        return basis, np.dot(null.T, np.dot(self._kernel(ctrl, ctrl), null))

    def transform_basis(self, basis):
        return np.dot(basis, np.r_[self.a, self.v])

    def _transform(self, points):
        basis, _ = self.prepare(points)
        return self.transform_basis(basis)

    def field_weights(self):
        """``N v``: the warp coefficients per control point (K, dim), ``N`` the null-space basis of ``prepare``."""
        ctrl = np.asarray(self.control_pts, dtype=np.float64)
        u, _, _ = np.linalg.svd(np.c_[np.ones((ctrl.shape[0], 1)), ctrl])
        return np.dot(u[:, ctrl.shape[1] + 1:], np.asarray(self.v, dtype=np.float64))

    def warp(self, points):
        """``[1 x] a + sum_k U(|x - c_k|) (N v)_k`` with the kernel sum on the GPU in fp64: no Q x K matrix is formed.  An
        object built with a kernel of its own has no device counterpart and goes through ``transform``."""
        if self._kernel is not _tps_kernel:
            return self.transform(points)
        ctrl = np.asarray(self.control_pts, dtype=np.float64)
        pts = _warp_points(points, ctrl.shape[1])
        a = np.asarray(self.a, dtype=np.float64)
        return a[0] + np.dot(pts, a[1:]) + _field(self, ctrl, self.field_weights(), "tps").evaluate(pts)

    def close(self):
        """Release the GPU handle that ``warp`` keeps."""
        _close_field(self)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the library may be gone already
            pass


# ---- dual quaternions: 8 doubles (r_w, r_x, r_y, r_z, d_w, d_x, d_y, d_z) -------------------
def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def dualquat_identity(k=None):
    """The identity dual quaternion, or a (k, 8) array of them."""
    one = np.array([1.0, 0, 0, 0, 0, 0, 0, 0])
    return one if k is None else np.tile(one, (int(k), 1))


def dualquat_from_rt(rot, t):
    """Dual quaternion of x -> R x + t: ``rot`` a 3 x 3 rotation matrix or a unit quaternion (w, x, y, z); d = (0, t) r / 2."""
    rot = np.asarray(rot, dtype=np.float64)
    if rot.shape == (3, 3):
        # Shepperd's method: the largest of (1 + tr, 1 + 2 R_ii - tr) picks the pivot
        tr = np.trace(rot)
        cand = np.array([tr, rot[0, 0], rot[1, 1], rot[2, 2]])
        i = int(np.argmax(cand))
        if i == 0:
            r = np.array([1.0 + tr, rot[2, 1] - rot[1, 2], rot[0, 2] - rot[2, 0], rot[1, 0] - rot[0, 1]])
        else:
            a, b, c = i - 1, i % 3, (i + 1) % 3
            r = np.zeros(4)
            r[0] = rot[c, b] - rot[b, c]
            r[1 + a] = 1.0 + 2.0 * rot[a, a] - tr
            r[1 + b] = rot[b, a] + rot[a, b]
            r[1 + c] = rot[c, a] + rot[a, c]
        r = r / np.linalg.norm(r)
    else:
        r = rot.reshape(4)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    return np.r_[r, 0.5 * _quat_mul(np.r_[0.0, t], r)]


def dualquat_from_twist(tw):
    """Reference filterreg.py:38-42: rotation by ``|tw[:3]|`` about ``tw[:3]`` (the identity below float32 eps), translation ``tw[3:]``."""
    tw = np.asarray(tw, dtype=np.float64)
    ang = np.linalg.norm(tw[:3])
    if ang < np.finfo(np.float32).eps:
        return dualquat_from_rt(np.array([1.0, 0.0, 0.0, 0.0]), tw[3:])
    return dualquat_from_rt(np.r_[np.cos(0.5 * ang), np.sin(0.5 * ang) * tw[:3] / ang], tw[3:])


def dualquat_mul(a, b):
    """``a * b`` (applies ``b`` first): r = a.r b.r, d = a.r b.d + a.d b.r."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.r_[_quat_mul(a[:4], b[:4]), _quat_mul(a[:4], b[4:]) + _quat_mul(a[4:], b[:4])]


class DeformableKinematicModel(Transformation):
    """Dual-quaternion skinning, two nodes per point (reference transformation.py:163-212).

    dualquats : (K, 8) float64 array or a sequence of K length-8 arrays (r_w, r_x, r_y, r_z, d_w, d_x, d_y, d_z) -
                NOT ``dq3d`` objects (known deviation; ``dualquat_from_rt`` / ``dualquat_from_twist`` build them)
    weights   : ``DeformableKinematicModel.SkinningWeight`` (``make_weight(pairs, vals)``)

    Point i moves by the blend ``val[0] * dualquats[pair[0]] + val[1] * dualquats[pair[1]]`` divided by the norm of
    its rotation part (DLB, no antipodal sign correction); ``transform`` runs on the GPU.
    """

    class SkinningWeight(np.ndarray):
        """Per point: two node indices ``['pair']`` (i4) and two weights ``['val']`` (f4)  (transformation.py:171-194)."""

        def __new__(cls, n_points):
            return super(DeformableKinematicModel.SkinningWeight, cls).__new__(
                cls, n_points, dtype=[("pair", "i4", 2), ("val", "f4", 2)]
            )

        @property
        def n_nodes(self):
            return int(self["pair"].max()) + 1

        def pairs_set(self):
            return itertools.permutations(range(self.n_nodes), 2)

        def in_pair(self, pair):
            """Indices of the points whose pair equals the given ordered pair."""
            return np.argwhere((self["pair"] == pair).all(1)).flatten()

    @classmethod
    def make_weight(cls, pairs, vals):
        pairs = np.asarray(pairs)
        weights = cls.SkinningWeight(pairs.shape[0])
        weights["pair"] = pairs
        weights["val"] = vals
        return weights

    def __init__(self, dualquats, weights):
        super(DeformableKinematicModel, self).__init__()
        self.weights = weights
        self.dualquats = np.array([np.asarray(q, dtype=np.float64).reshape(8) for q in dualquats]).reshape(-1, 8)
        pair = np.asarray(weights["pair"])
        if pair.size and (pair.min() < 0 or pair.max() >= self.dualquats.shape[0]):
            raise ValueError("skinning weights name a node outside [0, %d)." % self.dualquats.shape[0])

    def _transform(self, points):
        import ctypes

        from . import _lib
        from .engine import _current_device_and_stream

        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("DeformableKinematicModel moves (n, 3) points.")
        if points.shape[0] != self.weights.shape[0]:
            raise ValueError("%d points for %d skinning weights." % (points.shape[0], self.weights.shape[0]))
        _lib.require_gpu()
        dev, st = _current_device_and_stream()
        pairs = np.ascontiguousarray(self.weights["pair"], dtype=np.int32)
        vals = np.ascontiguousarray(self.weights["val"], dtype=np.float32)
        dq = np.ascontiguousarray(self.dualquats, dtype=np.float64)
        out = np.empty_like(points)
        _lib.check(_lib.lib.prg_dq_skin(dev, ctypes.c_void_p(st), _lib.ptr(points), points.shape[0], _lib.ptr(pairs),
                                        _lib.ptr(vals), _lib.ptr(dq), dq.shape[0], _lib.ptr(out)))
        return out
