"""Kernel fields: the displacement field of a non-rigid result, evaluated at any points.

``f(x)_c = sum_m k(|x - y_m|^2) w_mc`` over control points ``y_m`` with weight columns ``w``: what ``NonRigidTransformation``
(Gaussian), ``CombinedTransformation`` (inverse multiquadric) and ``TPSTransformation`` (thin-plate spline) hold at their
control points only.  The reference has no counterpart: it applies a result through the M x M (or Q x K) float32 kernel
matrix.  Here the sum runs in ``libprobreg_hip.so`` (``prg_field_*``, csrc/field.hip) in fp64 with a stated order, so the
results are byte-identical from run to run and do not depend on how many points are evaluated at once.

``Transformation.warp(points)`` is the interface most callers want; it moves any points with a finished registration::

    from probreg_amd import cpd, preprocess
    small = preprocess.voxel_down_sample(source, 0.05).points
    tf = cpd.registration_cpd(small, preprocess.voxel_down_sample(target, 0.05).points, "nonrigid").transformation
    moved = tf.warp(source)          # the full-resolution cloud, a mesh's vertices, landmarks ...
"""
import numpy as np

from . import _lib
from .preprocess import _single_process

KERNELS = {"gaussian": 0, "imq": 1, "tps": 2}  # PRG_FIELD_GAUSSIAN, PRG_FIELD_IMQ, PRG_FIELD_TPS
MAX_COLUMNS = 4


class KernelField(_lib.Handle):
    """``f(x) = sum_m k(|x - control_m|^2) weights_m`` on the GPU, in fp64.

    control : (M, D) array, D = 2 or 3;  weights : (M, C) array (or (M,) for C = 1), 1 <= C <= 4; both finite
    kernel  : "gaussian" - ``exp(-d2 / (2 param))``, param = beta > 0 (``math_utils.rbf_kernel``: 2 beta, not 2 beta^2)
              "imq"      - ``1 / sqrt(d2 + param)``, param = c > 0 (``math_utils.inverse_multiquadric_kernel``)
              "tps"      - ``math_utils.tps_kernel``: D = 2 ``d2 log(d2) / 2`` where d2 > 1e-9, else 0; D = 3 ``-sqrt(d2)``
    Everything is checked on the host before anything is launched; ``ValueError`` names the argument.
    """

    def __init__(self, control, weights, kernel, param=None, device=None):
        _single_process("KernelField")
        control, weights, kind, param = _check_control(control, weights, kernel, param)
        super().__init__(_lib.lib.prg_field_create, _lib.lib.prg_field_destroy, device)
        try:
            self._set(control, weights, kind, param)
        except Exception:
            self.close()
            raise

    def _set(self, control, weights, kind, param):
        _lib.check(_lib.lib.prg_field_set_control(self._h, _lib.ptr(control), _lib.ptr(weights), control.shape[0],
                                                  control.shape[1], weights.shape[1], kind, param))
        self.dim, self.columns = control.shape[1], weights.shape[1]

    def set_control(self, control, weights, kernel, param=None):
        """Other control points, weights or kernel on the same handle."""
        self._set(*_check_control(control, weights, kernel, param))

    def evaluate(self, points):
        """``f`` at ``points`` (Q, D) -> (Q, C) float64; Q = 0 gives an empty array without a launch."""
        pts = np.ascontiguousarray(_lib.as_points(points))
        if pts.ndim != 2 or pts.shape[1] != self.dim:
            raise ValueError("points must be (n, %d) like the control points, got shape %s" % (self.dim, pts.shape))
        if not np.all(np.isfinite(pts)):
            raise ValueError("points contains NaN or infinity")
        out = np.empty((pts.shape[0], self.columns), dtype=np.float64)
        if pts.shape[0]:
            _lib.check(_lib.lib.prg_field_evaluate(self._h, _lib.ptr(pts), pts.shape[0], _lib.ptr(out)))
        return out


def _check_control(control, weights, kernel, param):
    if kernel not in KERNELS:
        raise ValueError("kernel must be one of %s (got %r)" % (", ".join(repr(k) for k in KERNELS), kernel))
    control = _lib.as_cloud(control, "control", (2, 3))
    weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
    if weights.ndim == 1:
        weights = weights[:, None]
    if weights.ndim != 2 or weights.shape[0] != control.shape[0]:
        raise ValueError("weights must have one row per control point (%d), got shape %s" % (control.shape[0], weights.shape))
    if not 1 <= weights.shape[1] <= MAX_COLUMNS:
        raise ValueError("weights must have 1 .. %d columns, got %d" % (MAX_COLUMNS, weights.shape[1]))
    if not np.all(np.isfinite(weights)):
        raise ValueError("weights contains NaN or infinity")
    if kernel == "tps":
        if param is not None:
            raise ValueError("the tps kernel has no parameter (got param=%r)" % (param,))
        return control, weights, KERNELS[kernel], 0.0
    name = "beta" if kernel == "gaussian" else "c"
    try:
        value = float("nan") if param is None or isinstance(param, (bool, str, bytes)) else float(param)
    except (TypeError, ValueError):
        value = float("nan")
    if not (np.isfinite(value) and value > 0.0):
        raise ValueError("%s (param) of the %s kernel must be a finite number > 0, got %r" % (name, kernel, param))
    return control, weights, KERNELS[kernel], value
