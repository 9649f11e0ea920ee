"""NumPy stand-in for the ``dq3d`` package (``quat``, ``dualquat``, ``op.dlb``) with the conventions of DESIGN.md
section 3.10, so that the reference's deformable kinematic code can be executed where ``dq3d`` is not installed.

TEST INFRASTRUCTURE.  ``register()`` puts it into ``sys.modules`` as ``dq3d`` and ``dq3d.op``.  What ``dq3d`` itself
does with an unnormalised blend cannot be checked without the package: the normalised form is the definition here.
"""
import sys
import types

import numpy as np

import oracle_kinematic as ok


class quat(object):
    """Rotation quaternion (w, x, y, z); ``quat(angle, axis)`` as the reference calls it (filterreg.py:42)."""

    def __init__(self, *args):
        if len(args) == 2:
            ang, axis = float(args[0]), np.asarray(args[1], dtype=np.float64)
            self.data = np.r_[np.cos(0.5 * ang), np.sin(0.5 * ang) * axis]
        elif len(args) == 4:
            self.data = np.array(args, dtype=np.float64)
        else:
            self.data = np.asarray(args[0], dtype=np.float64).reshape(4).copy()

    @staticmethod
    def identity():
        return quat(1.0, 0.0, 0.0, 0.0)


class dualquat(object):
    """``dualquat(quat, translation)`` or ``dualquat(array of 8)``; ``.data`` = (r, d)."""

    def __init__(self, *args):
        if len(args) == 2:
            r = args[0].data if isinstance(args[0], quat) else np.asarray(args[0], dtype=np.float64)
            self.data = ok.dq_from_rt(r, np.asarray(args[1], dtype=np.float64))
        else:
            self.data = np.asarray(args[0], dtype=np.float64).reshape(8).copy()

    @staticmethod
    def identity():
        return dualquat(np.array([1.0, 0, 0, 0, 0, 0, 0, 0]))

    def __mul__(self, other):
        if isinstance(other, dualquat):
            return dualquat(ok.dq_mul(self.data, other.data))
        return dualquat(self.data * float(other))

    def __rmul__(self, scalar):
        return dualquat(self.data * float(scalar))

    def __add__(self, other):
        return dualquat(self.data + other.data)

    def normalized(self):
        return dualquat(self.data / ok.rnorm(self.data[:4]))

    def transform_point(self, p):
        return ok.dq_transform(self.normalized().data, np.asarray(p, dtype=np.float64))

    def __repr__(self):
        return "dualquat(%r)" % (self.data,)


def dlb(weights, dualquats):
    """Dual-quaternion linear blending, normalised, no antipodal sign correction."""
    acc = np.zeros(8)
    for w, q in zip(weights, dualquats):
        acc = acc + float(w) * q.data
    return dualquat(acc).normalized()


def register():
    mod = types.ModuleType("dq3d")
    op = types.ModuleType("dq3d.op")
    op.dlb = dlb
    mod.quat, mod.dualquat, mod.op = quat, dualquat, op
    sys.modules["dq3d"] = mod
    sys.modules["dq3d.op"] = op
    return mod
