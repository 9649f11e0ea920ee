"""``probreg.math_utils`` counterparts that are on the hot path (reference probreg/math_utils.py:28-37)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, lib, ptr
from .engine import _current_device_and_stream


def squared_kernel_sum(x, y):
    """sum_{m,n} |x_m - y_n|^2 / (M*D*N)  (reference math_utils.py:28-29 -> cc/math_utils.cc:5-15).

    Evaluated on the GPU in closed form in fp64, ``n sum|x|^2 + m sum|y|^2 - 2 sum x . sum y`` - the M x N float32 matrix of the
    reference is never built.  The three terms cancel, so the mean of all points is subtracted from both clouds in fp64 first
    (the quantity is a sum of squared differences: a common shift does not change it) and the kernels read fp64 coordinates:
    clouds of any dimension, at any distance from the origin, give the pairwise sum of the arrays as passed to ~1e-12
    relative.  (The reference rounds the coordinates to float32 and sums in float32: ~1e-7 relative near the origin.)
    """
    _lib.require_gpu()
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
        raise ValueError("x and y must be 2-D with the same number of columns.")
    if x.shape[0] and y.shape[0]:
        c = (x.sum(axis=0) + y.sum(axis=0)) / (x.shape[0] + y.shape[0])
        x = x - c
        y = y - c
    x = np.ascontiguousarray(x)
    y = np.ascontiguousarray(y)
    dev, st = _current_device_and_stream()
    out = ctypes.c_double(0.0)
    check(lib.prg_squared_kernel_sum(dev, ctypes.c_void_p(st), ptr(x), x.shape[0], ptr(y), y.shape[0], x.shape[1],
                                     ctypes.byref(out)))
    return float(out.value)


def rbf_kernel(x, y, beta):
    """K_ij = exp(-|x_i - y_j|^2 / (2*beta)) as float32 (reference math_utils.py:36-37 -> cc/math_utils.cc:17-19)."""
    _lib.require_gpu()
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
        raise ValueError("x and y must be 2-D with the same number of columns.")
    dev, st = _current_device_and_stream()
    out = np.empty((x.shape[0], y.shape[0]), dtype=np.float32)
    check(lib.prg_rbf_kernel(dev, ctypes.c_void_p(st), ptr(x), x.shape[0], ptr(y), y.shape[0], x.shape[1],
                             float(beta), ptr(out)))
    return out


def tps_kernel(x, y):
    """Thin-plate-spline kernel as float32 (reference math_utils.py:40-47 -> cc/math_utils.cc:21-30): 2-D
    ``r^2 log r`` (0 where r^2 <= 1e-9), 3-D ``-r``.  K x K and M x K on mixture components: host NumPy."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
        raise ValueError("x and y must be 2-D with the same number of columns.")
    if x.shape[1] not in (2, 3):
        raise ValueError("Invalid dimension of x: %d." % x.shape[1])
    d2 = np.zeros((x.shape[0], y.shape[0]), dtype=np.float32)
    for k in range(x.shape[1]):
        d = x[:, k, None] - y[None, :, k]
        d2 += d * d
    if x.shape[1] == 3:
        return -np.sqrt(d2)
    out = np.zeros_like(d2)
    far = d2 > np.float32(1.0e-9)
    out[far] = d2[far] * np.log(np.sqrt(d2[far]))
    return out


def inverse_multiquadric_kernel(x, y, c=1.0):
    """K_ij = 1 / sqrt(|x_i - y_j|^2 + c) as float32 (reference math_utils.py:50-51 -> cc/math_utils.cc:32-34)."""
    _lib.require_gpu()
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
        raise ValueError("x and y must be 2-D with the same number of columns.")
    dev, st = _current_device_and_stream()
    out = np.empty((x.shape[0], y.shape[0]), dtype=np.float32)
    check(lib.prg_inverse_multiquadric_kernel(dev, ctypes.c_void_p(st), ptr(x), x.shape[0], ptr(y), y.shape[0],
                                              x.shape[1], float(c), ptr(out)))
    return out


def compute_rmse(source, target):
    """Mean distance from every source point to its nearest target point (reference math_utils.py:32-33).

    The reference takes a prebuilt ``cKDTree`` of the target; here ``target`` is the point array itself (an object
    with a ``.data`` attribute, such as a cKDTree, is accepted too) and the search is a brute-force GPU sweep.
    Both clouds are shifted by the target centroid in float64 before the float32 upload.
    """
    _lib.require_gpu()
    tgt = np.asarray(getattr(target, "data", target), dtype=np.float64)
    src = np.asarray(source, dtype=np.float64)
    if src.ndim != 2 or tgt.ndim != 2 or src.shape[1] != tgt.shape[1]:
        raise ValueError("source and target must be 2-D with the same number of columns.")
    c = tgt.mean(axis=0)
    a = np.ascontiguousarray(src - c, dtype=np.float32)
    b = np.ascontiguousarray(tgt - c, dtype=np.float32)
    dev, st = _current_device_and_stream()
    out = ctypes.c_double(0.0)
    check(lib.prg_nn_mean_distance(dev, ctypes.c_void_p(st), ptr(a), a.shape[0], ptr(b), b.shape[0], a.shape[1],
                                   ctypes.byref(out)))
    return float(out.value)
