"""Writes tests/golden/kinematic_golden.npz from the UNMODIFIED reference (build container only): the reference's
``DeformableKinematicModel`` and ``DeformableKinematicFilterReg`` on its own example (examples/filterreg_deformable.py),
executed with the NumPy stand-in for ``dq3d`` (tests/dq3d_standin.py, conventions of DESIGN.md section 3.10).

    python tests/golden/make_kinematic_golden.py

The file holds data only: inputs, the transformed points, one M-step from the identity on exact correspondences
(m0 = 1, m1 = the transformed points, float64) and one expectation_step at sigma2 = 0.01.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dq3d_standin  # noqa: E402

dq3d = dq3d_standin.register()  # before the reference is imported: it then reports _imp_dq True

from oracle import ref_import  # noqa: E402


def main():
    ref = ref_import.load(with_filterreg=True)
    assert ref.filterreg._imp_dq and ref.transformation._imp_dq
    n = 30
    points = np.array([[i * 0.05, 0.0, 0.0] for i in range(n)])
    dqs = [dq3d.dualquat(dq3d.quat(np.deg2rad(0.0), np.array([0.0, 0.0, 1.0])), np.array([0.0, 0.0, 0.0])),
           dq3d.dualquat(dq3d.quat(np.deg2rad(30.0), np.array([0.0, 0.0, 1.0])), np.array([0.0, 0.0, 0.3]))]
    ws = ref.transformation.DeformableKinematicModel.SkinningWeight(n)
    for i in range(n):
        ws["pair"][i] = (0, 1)
        ws["val"][i] = (float(i) / n, 1.0 - float(i) / n)
    model = ref.transformation.DeformableKinematicModel(dqs, ws)
    moved = model.transform(points)

    reg = ref.filterreg.DeformableKinematicFilterReg(points, ws, 0.01)
    es = ref.filterreg.EstepResult(np.ones(n), moved.copy(), None, None)
    res = reg.maximization_step(points, moved, es)
    out_dq = np.array([q.data for q in res.transformation.dualquats])
    out_pts = res.transformation.transform(points)

    est = reg.expectation_step(points, moved, moved, 0.01, True)
    out = {
        "example/source": points, "example/pairs": np.asarray(ws["pair"]), "example/vals": np.asarray(ws["val"]),
        "example/dualquats": np.array([q.data for q in dqs]), "example/transformed": np.asarray(moved),
        "example/mstep_dualquats": out_dq, "example/mstep_q": np.float64(res.q), "example/mstep_sigma2": np.float64(res.sigma2),
        "example/mstep_transformed": np.asarray(out_pts),
        "example/estep_sigma2": np.float64(0.01), "example/estep_m0": np.asarray(est.m0), "example/estep_m1": np.asarray(est.m1),
        "example/estep_m2": np.asarray(est.m2),
    }
    path = os.path.join(HERE, "kinematic_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "q =", res.q, "max err of the M-step", np.max(np.abs(out_pts - moved)))


if __name__ == "__main__":
    main()
