#!/usr/bin/env python
"""Generate tests/golden/field_golden.npz from the UNMODIFIED reference (``oracle.ref_import``), on the CPU:

    python tests/golden/make_field_golden.py

The file pins tests/oracle_field.py, the restatement of the kernel field of DESIGN.md section 3.18, on what the reference itself
computes through its float32 kernel matrices.  Vectors only (no kernel matrix is stored):

  cpd/   ``NonRigidCPD(beta=2, lmd=2).registration`` on the voxel means (edge 0.12) of ``synthetic.nonrigid_pair(3000, 3000,
         seed=1)``: control points, ``w``, beta and the moved control points ``transform(control)``.
  bcpd/  one ``CombinedBCPD`` M-step on the same means: ``nu``, the residual, ``s2s2``, lmd and the ``v_hat`` it returns.  The
         kernel matrix of these means has a condition number near 1e12 and the reference inverts it in float32.
  bcpd_grid/  the same on ``make_golden.bcpd_grid_pair(32, 6, 5, 4)``, 120 well-separated points whose kernel matrix the
         reference can invert.
  tps2/, tps3/  ``TPSTransformation(a, v, control).transform(points)`` on points that are not the control points.

``probreg._math.tps_kernel_2d / _3d`` are the float32 restatements of cc/math_utils.cc:21-30 (as in make_gmmreg_golden.py).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

sys.path.insert(0, HERE)

from make_golden import bcpd_grid_pair  # noqa: E402
from oracle import ref_import  # noqa: E402
from probreg_amd import synthetic  # noqa: E402

OUT = os.path.join(HERE, "field_golden.npz")
VOXEL = 0.12


def _sqdist_f32(x, y):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    k = np.zeros((x.shape[0], y.shape[0]), dtype=np.float32)
    for d in range(x.shape[1]):
        e = x[:, d, None] - y[None, :, d]
        k += e * e
    return k


def tps_kernel_2d(x, y):  # cc/math_utils.cc:21-26
    d2 = _sqdist_f32(x, y)
    out = np.zeros_like(d2)
    m = d2 > np.float32(1.0e-9)
    out[m] = d2[m] * np.log(np.sqrt(d2[m]))
    return out


def tps_kernel_3d(x, y):  # cc/math_utils.cc:28-30
    return -np.sqrt(_sqdist_f32(x, y))


def voxel_means(points, v):
    """Open3D's voxel_down_sample on the host: cells floor((p - (min - v / 2)) / v), one mean per occupied cell, the cells in
    ascending (c_x, c_y, c_z) (the order of preprocess.voxel_down_sample)."""
    cells = np.floor((points - (points.min(axis=0) - 0.5 * v)) / v).astype(np.int64)
    _, inverse, counts = np.unique(cells, axis=0, return_inverse=True, return_counts=True)
    sums = np.zeros((counts.shape[0], points.shape[1]))
    np.add.at(sums, inverse.ravel(), points)
    return sums / counts[:, None]


def main():
    ref = ref_import.load()
    bc = ref_import.load_bcpd()
    sys.modules["probreg._math"].tps_kernel_2d = tps_kernel_2d
    sys.modules["probreg._math"].tps_kernel_3d = tps_kernel_3d
    data = {}

    src_full, tgt_full = synthetic.nonrigid_pair(3000, 3000, seed=1)
    src, tgt = voxel_means(src_full, VOXEL), voxel_means(tgt_full, VOXEL)

    reg = ref.cpd.NonRigidCPD(src.copy(), beta=2.0, lmd=2.0)
    res = reg.registration(tgt.copy(), maxiter=40, tol=1e-6)
    data["cpd/control"], data["cpd/w"], data["cpd/beta"] = src, np.asarray(res.transformation.w), np.asarray(2.0)
    data["cpd/moved"] = res.transformation.transform(src)
    print("cpd   M=%d max|w|=%.3g max|disp|=%.3g" % (src.shape[0], np.abs(data["cpd/w"]).max(),
                                                    np.abs(data["cpd/moved"] - src).max()))

    for pre, (bs, bt) in (("bcpd/", (src, tgt)), ("bcpd_grid/", bcpd_grid_pair(32, nx=6, ny=5, nz=4, extra=25))):
        b = bc.CombinedBCPD(bs.copy(), lmd=2.0)
        init = b._initialize(bt)
        es = b.expectation_step(bs, bt, 1.0, init.alpha, init.sigma_mat, init.sigma2, 0.0)
        rigid = init.transformation.rigid_trans
        ms = b.maximization_step(bt, rigid, es, init.sigma2)
        data[pre + "control"], data[pre + "nu"] = bs, np.asarray(es.nu)
        data[pre + "residual"] = rigid.inverse().transform(es.x_hat) - bs                                # bcpd.py:132
        data[pre + "s2s2"], data[pre + "lmd"] = np.asarray(rigid.scale ** 2 / init.sigma2 ** 2), np.asarray(2.0)  # bcpd.py:129
        data[pre + "v_hat"] = np.asarray(ms.transformation.v)
        print("%-10s M=%d s2s2=%.4g max|v_hat|=%.3g cond(G)=%.3g" % (pre, bs.shape[0], float(data[pre + "s2s2"]),
                                                                      np.abs(data[pre + "v_hat"]).max(),
                                                                      np.linalg.cond(b.gmat.astype(np.float64))))

    rng = np.random.default_rng(7)
    for dim in (2, 3):
        k = 40
        control = rng.uniform(-1.0, 1.0, (k, dim))
        a = np.r_[rng.normal(0.0, 0.05, (1, dim)), np.identity(dim) + rng.normal(0.0, 0.05, (dim, dim))]
        v = rng.normal(0.0, 0.05, (k - dim - 1, dim))
        points = rng.uniform(-1.2, 1.2, (150, dim))
        trans = ref.transformation.TPSTransformation(a, v, control)
        pre = "tps%d/" % dim
        data[pre + "control"], data[pre + "a"], data[pre + "v"], data[pre + "points"] = control, a, v, points
        data[pre + "moved"] = trans.transform(points)
        print("tps%d  K=%d Q=%d" % (dim, k, points.shape[0]))

    np.savez_compressed(OUT, **data)
    print("wrote %s (%d arrays, %.1f KB)" % (OUT, len(data), os.path.getsize(OUT) / 1024.0))


if __name__ == "__main__":
    main()
