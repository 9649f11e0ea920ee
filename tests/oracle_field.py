"""NumPy fp64 restatement of the kernel field of DESIGN.md section 3.18 and the error bounds its tests assert.

``f(x)_c = sum_m k(|x - y_m|^2) w_mc``: differences, squared distance, kernel and sums in fp64 straight from the coordinates,
control points in ascending index, slabs of 65 536 summed from 0 and added in ascending slab order.  Nothing here touches the
GPU or the library.
"""
import numpy as np

SLAB = 65536
KERNELS = ("gaussian", "imq", "tps")
TPS_EPS = 1.0e-9  # math_utils.tps_kernel: the 2-D spline is 0 where d2 <= 1e-9


def _prepare(points, control, weights):
    x = np.asarray(points, dtype=np.float64)
    y = np.asarray(control, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    if w.ndim == 1:
        w = w[:, None]
    assert x.ndim == 2 and y.ndim == 2 and x.shape[1] == y.shape[1] and x.shape[1] in (2, 3)
    assert w.shape[0] == y.shape[0]
    return x, y, w


def sqdist(x, y):
    """(Q, M) squared distances, the axes added in ascending order."""
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for a in range(x.shape[1]):
        e = x[:, a, None] - y[None, :, a]
        d2 += e * e
    return d2


def kernel_value(d2, kernel, param, dim):
    """k(d2)."""
    if kernel == "gaussian":
        return np.exp(-d2 / (2.0 * param))
    if kernel == "imq":
        return 1.0 / np.sqrt(d2 + param)
    assert kernel == "tps"
    if dim == 3:
        return -np.sqrt(d2)
    out = np.zeros_like(d2)
    far = d2 > TPS_EPS
    out[far] = 0.5 * d2[far] * np.log(d2[far])
    return out


def kernel_sensitivity(d2, kernel, param, dim):
    """d2 |k'(d2)|: what a relative error of d2 does to k."""
    if kernel == "gaussian":
        return d2 / (2.0 * param) * np.exp(-d2 / (2.0 * param))
    if kernel == "imq":
        return 0.5 * d2 * (d2 + param) ** -1.5
    if dim == 3:
        return 0.5 * np.sqrt(d2)
    out = np.zeros_like(d2)
    far = d2 > TPS_EPS
    out[far] = 0.5 * d2[far] * np.abs(np.log(d2[far]) + 1.0)
    return out


def field(points, control, weights, kernel, param=None):
    """(Q, C) field values in the order of the definition (``np.cumsum`` adds sequentially, unlike ``np.sum``)."""
    x, y, w = _prepare(points, control, weights)
    out = np.zeros((x.shape[0], w.shape[1]))
    for s0 in range(0, y.shape[0], SLAB):
        k = kernel_value(sqdist(x, y[s0:s0 + SLAB]), kernel, param, x.shape[1])
        part = np.stack([np.cumsum(k * w[None, s0:s0 + SLAB, c], axis=1)[:, -1] for c in range(w.shape[1])], axis=1)
        out = part if s0 == 0 else out + part
    return out


def bound(points, control, weights, kernel, param=None):
    """A-priori error bound per output: ``2^-53 sum_m [(M + 64) |k| + 4 d2 |k'|] |w_mc|`` - any summation order of M terms
    plus a few ulp in the kernel function, and the kernel's response to 4 ulp in d2."""
    x, y, w = _prepare(points, control, weights)
    m = y.shape[0]
    out = np.zeros((x.shape[0], w.shape[1]))
    for s0 in range(0, m, SLAB):
        d2 = sqdist(x, y[s0:s0 + SLAB])
        dim = x.shape[1]
        term = (m + 64.0) * np.abs(kernel_value(d2, kernel, param, dim)) + 4.0 * kernel_sensitivity(d2, kernel, param, dim)
        out += term @ np.abs(w[s0:s0 + SLAB])
    return out * 2.0 ** -53


def bcpd_weights(s2s2, lmd, nu, residual, v_hat):
    """W_b with v_hat = G W_b: from Sigma^-1 v_hat = s2s2 nu o residual and Sigma^-1 = lmd G^-1 + s2s2 diag(nu)."""
    nu = np.asarray(nu, dtype=np.float64)
    return (s2s2 / lmd) * nu[:, None] * (np.asarray(residual, dtype=np.float64) - np.asarray(v_hat, dtype=np.float64))


def kernel_matrix_f32(x, y, kernel, param=None):
    """The float32 kernel matrix the reference applies a result through (cc/math_utils.cc: rbfKernel with 2 beta,
    inverseMultiQuadricKernel, tpsKernel2d / 3d), everything in float32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    d2 = np.zeros((x.shape[0], y.shape[0]), dtype=np.float32)
    for a in range(x.shape[1]):
        e = x[:, a, None] - y[None, :, a]
        d2 += e * e
    if kernel == "gaussian":
        return np.exp(-d2 / np.float32(2.0 * param)).astype(np.float32)
    if kernel == "imq":
        return (np.float32(1.0) / np.sqrt(d2 + np.float32(param))).astype(np.float32)
    assert kernel == "tps"
    if x.shape[1] == 3:
        return -np.sqrt(d2)
    out = np.zeros_like(d2)
    far = d2 > np.float32(TPS_EPS)
    out[far] = d2[far] * np.log(np.sqrt(d2[far]))
    return out


def f32_kernel_bound(points, control, weights, kernel, param=None):
    """``3 2^-24 sum_m |G_im| |w_mc|``: the distance of a sum taken through a float32 kernel matrix (float32 coordinates, d2 and
    kernel function: three roundings of relative size 2^-24 per entry) from the fp64 field."""
    x, y, w = _prepare(points, control, weights)
    g = np.abs(kernel_value(sqdist(x, y), kernel, param, x.shape[1]))
    return 3.0 * 2.0 ** -24 * (g @ np.abs(w))
