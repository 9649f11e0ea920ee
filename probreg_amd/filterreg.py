"""FilterReg (rigid, point-to-point) on MI355X - drop-in for ``probreg.filterreg`` on that path
(reference probreg/filterreg.py:27-196, 269-317).

The E-step (lattice build over [t_source; target]/sigma, the three Gaussian filters) and the M-step
(weighted Kabsch, composition, sigma2 update) run in ``libprobreg_hip.so``; the Python loop mirrors
``FilterReg.registration`` (filterreg.py:120-147) line by line, including its quirks: with the defaults
sigma2 is never updated, the returned ``sigma2`` is the un-clamped one, and the driver stops with the
previous ``q`` when every ``m0`` is zero.
Point-to-plane (``objective_type='pt2pl'``, filterreg.py:183-186 + cc/point_to_plane.cc) is built as well, and so are
feature-space lattices: a ``feature_fn`` other than the identity (filterreg.py:121, 125-133; e.g. 33-dimensional FPFH
descriptors) runs the reference's loop - transform, ``feature_fn`` on the host, lattice E-step over the features
(1 <= d <= 64) and M-step on the GPU.

``DeformableKinematicFilterReg`` (filterreg.py:199-266) moves the source by dual-quaternion skinning, two nodes per point
(``transformation.DeformableKinematicModel``).  Its M-step is the COMPLETE Gauss-Newton system of DESIGN.md section 3.10
- the reference fills only the off-diagonal node blocks and diverges on anything but its own example; that system stays
available as ``reference_form=True``.  Skinning, the lattice E-step and the per-node-pair sums of the M-step run on the
GPU and stay there over the EM loop; the 6K x 6K assembly and the minimum-norm solve are host LAPACK.
"""
import abc
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from . import math_utils as mu
from . import transformation as tf
from ._lib import as_points as _as_points
from ._lib import check, lib, ptr
from .engine import _current_device_and_stream
from .log import log

EstepResult = namedtuple("EstepResult", ["m0", "m1", "m2", "nx"])
MstepResult = namedtuple("MstepResult", ["transformation", "sigma2", "q"])
MstepResult.__doc__ = """(transformation, sigma2, q) of one FilterReg M-step / of the whole registration (reference filterreg.py:28)."""


def _identity(x):
    return x


class _Plan(_lib.Handle):
    """One ``prg_filterreg`` handle."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_fr_create, _lib.lib.prg_fr_destroy, device)
        self.m = self.n = self.dim = 0

    def set_source(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.m, self.dim = a.shape
        check(lib.prg_fr_set_source(self._h, ptr(a), a.shape[0], a.shape[1]))

    def set_target(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.n = a.shape[0]
        check(lib.prg_fr_set_target(self._h, ptr(a), a.shape[0], a.shape[1]))

    def set_state(self, rot, t, sigma2):
        r = np.identity(3)
        d = np.asarray(rot).shape[0]
        r[:d, :d] = rot
        tt = np.zeros(3)
        tt[:d] = t
        check(lib.prg_fr_set_state(self._h, ptr(np.ascontiguousarray(r)), ptr(tt), float(sigma2)))

    def estep(self, alpha=0.015):
        size, blur = ctypes.c_int(0), ctypes.c_int(0)
        check(lib.prg_fr_estep(self._h, float(alpha), ctypes.byref(size), ctypes.byref(blur)))
        return int(size.value), bool(blur.value)

    def get_estep(self, want_m2):
        m0 = np.empty(self.m, dtype=np.float32)
        m1 = np.empty((self.m, self.dim), dtype=np.float32)
        m2 = np.empty(self.m, dtype=np.float32) if want_m2 else None
        check(lib.prg_fr_get_estep(self._h, ptr(m0), ptr(m1), ptr(m2) if want_m2 else None))
        return m0, m1, m2

    def set_normals(self, normals):
        if normals is None:
            check(lib.prg_fr_set_target_normals(self._h, None))
        else:
            a = np.ascontiguousarray(normals, dtype=np.float64)
            if a.shape != (self.n, 3):
                raise ValueError("target_normals must be an (n, 3) array matching the target.")
            check(lib.prg_fr_set_target_normals(self._h, ptr(a)))

    def get_nx(self):
        nx = np.empty((self.m, 3), dtype=np.float32)
        check(lib.prg_fr_get_nx(self._h, ptr(nx)))
        return nx

    def mstep(self, w, update_sigma2, objective_type="pt2pt", min_sigma2=-1.0, read=True):
        """``min_sigma2`` >= 0 advances the device sigma2 like the driver (filterreg.py:140); negative leaves it alone.
        ``read=False`` only enqueues the M-step (no read-back, the host does not wait) and returns None."""
        fn = lib.prg_fr_mstep_pt2pl if objective_type == "pt2pl" else lib.prg_fr_mstep
        if not read:
            check(fn(self._h, float(w), 1 if update_sigma2 else 0, float(min_sigma2), None))
            return None
        out = np.zeros(18)
        check(fn(self._h, float(w), 1 if update_sigma2 else 0, float(min_sigma2), ptr(out)))
        return out

    def get_state(self):
        """The 20-double device state (prg_fr_get_state); synchronises."""
        out = np.zeros(20)
        check(lib.prg_fr_get_state(self._h, ptr(out)))
        return out

    def last_route(self):
        """(route, lattice builds, table attempts of the last build, sampled) of the last E-step (prg_fr_last_route)."""
        out = (ctypes.c_int * 4)()
        check(lib.prg_fr_last_route(self._h, out))
        return tuple(int(v) for v in out)

    # ---- deformable kinematic model ----
    def set_skinning(self, pairs, vals, n_nodes):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float32)
        nseg = ctypes.c_int(0)
        check(lib.prg_fr_set_skinning(self._h, ptr(pairs), ptr(vals), pairs.shape[0], int(n_nodes), ctypes.byref(nseg)))
        self.n_nodes = int(n_nodes)
        # the segments of the device sums: the distinct ordered pairs, ascending in pair0 * K + pair1
        keys = np.unique(pairs[:, 0].astype(np.int64) * int(n_nodes) + pairs[:, 1])
        assert keys.shape[0] == nseg.value
        self.seg_a, self.seg_b = keys // int(n_nodes), keys % int(n_nodes)

    def set_dualquats(self, dq):
        dq = np.ascontiguousarray(dq, dtype=np.float64)
        check(lib.prg_fr_set_dualquats(self._h, ptr(dq), dq.shape[0]))

    def get_dualquats(self):
        dq = np.empty((self.n_nodes, 8))
        check(lib.prg_fr_get_dualquats(self._h, ptr(dq), self.n_nodes))
        return dq

    def kinematic_estep(self, sigma2, alpha=0.015):
        size, blur = ctypes.c_int(0), ctypes.c_int(0)
        check(lib.prg_fr_kinematic_estep(self._h, float(sigma2), float(alpha), ctypes.byref(size), ctypes.byref(blur)))
        return int(size.value), bool(blur.value)

    def kinematic_set_arrays(self, t_source, m0, m1, m2, n_target):
        check(lib.prg_fr_kinematic_set_arrays(self._h, ptr(t_source), ptr(m0), ptr(m1), None if m2 is None else ptr(m2),
                                              int(n_target)))

    def kinematic_normal_sums(self, sigma2, w, reference_form):
        out = np.empty((self.seg_a.shape[0], 34))
        check(lib.prg_fr_kinematic_normal_sums(self._h, float(sigma2), float(w), 1 if reference_form else 0, out.shape[0],
                                               ptr(out)))
        return out

    def kinematic_grad_sums(self, tw, reference_form):
        tw = np.ascontiguousarray(tw, dtype=np.float64)
        out = np.empty((self.seg_a.shape[0], 16))
        check(lib.prg_fr_kinematic_grad_sums(self._h, ptr(tw), 1 if reference_form else 0, out.shape[0], ptr(out)))
        return out


class FilterReg(abc.ABC):
    """Gaussian-filter based EM registration, driver part (reference filterreg.py:45-147).

    source         : (M, D) array that gets moved
    target_normals : (N, 3) unit normals of the target, only for ``objective_type='pt2pl'``
    sigma2         : kernel variance; ``None`` = mean squared source-target distance (clamped to ``min_sigma2``)
    update_sigma2  : re-estimate sigma2 in every M-step (off by default, as in the reference)
    """

    def __init__(self, source=None, target_normals=None, sigma2=None, update_sigma2=False):
        self._source = _as_points(source)
        self._target_normals = target_normals
        self._sigma2 = sigma2
        self._update_sigma2 = update_sigma2
        self._tf_type = None
        self._tf_result = None
        self._callbacks = []
        self._plan = None

    def set_source(self, source):
        self._source = _as_points(source)

    def set_target_normals(self, target_normals):
        self._target_normals = target_normals

    def set_callbacks(self, callbacks):
        self._callbacks = callbacks

    def _ensure_plan(self, target):
        if self._plan is None:
            self._plan = _Plan()
        self._plan.set_source(self._source)
        self._plan.set_target(target)
        return self._plan

    def expectation_step(self, t_source, target, y, sigma2, update_sigma2, objective_type="pt2pt", alpha=0.015):
        """Expectation step (reference filterreg.py:78-108) on explicit arrays; returns float32 m0, m1, m2 (, nx).

        ``t_source`` / ``target`` are the FEATURES the lattice is built over (the transformed source and the target
        themselves for the identity ``feature_fn``, anything up to 64-dimensional otherwise) and ``y`` the target
        positions whose moments are filtered.
        """
        t_source, target, y = np.asarray(t_source), np.asarray(target), np.asarray(y)
        assert t_source.ndim == 2 and target.ndim == 2, "source and target must have 2 dimensions."
        if objective_type not in ("pt2pt", "pt2pl"):
            raise ValueError("Unknown objective_type: %s." % objective_type)
        if t_source.shape[1] <= 3 and y.shape == target.shape and np.array_equal(y, target):
            # positions as features: the fused plan (one lattice pass for all channels)
            plan = _Plan()
            try:
                plan.set_source(t_source)
                plan.set_target(target)
                if objective_type == "pt2pl":
                    plan.set_normals(self._target_normals)
                plan.set_state(np.identity(t_source.shape[1]), np.zeros(t_source.shape[1]), sigma2)
                plan.estep(alpha)
                m0, m1, m2 = plan.get_estep(update_sigma2)
                nx = plan.get_nx() if objective_type == "pt2pl" else None
            finally:
                plan.close()
            return EstepResult(m0, m1, m2, nx)
        return self._expectation_step_features(t_source, target, y, sigma2, update_sigma2, objective_type, alpha)

    def _expectation_step_features(self, fsource, ftarget, y, sigma2, update_sigma2, objective_type, alpha):
        """filterreg.py:78-108 line by line on ``gaussian_filtering.Permutohedral`` (GPU lattice of any d <= 64)."""
        from . import gaussian_filtering as gf

        m, n = fsource.shape[0], ftarget.shape[0]
        sigma = np.sqrt(sigma2)
        fin = np.r_[fsource / sigma, ftarget / sigma]
        ph = gf.Permutohedral(fin)
        if ph.get_lattice_size() > n * alpha:  # :90-91
            ph = gf.Permutohedral(fin, False)
        zeros_m1 = np.zeros((m, 1))
        m0 = ph.filter(np.r_[zeros_m1, np.ones((n, 1))], m).flatten()[:m]
        m1 = ph.filter(np.r_[np.zeros((m, y.shape[1])), y], m)[:m]
        m2 = ph.filter(np.r_[zeros_m1, np.square(y).sum(axis=1)[:, None]], m).flatten()[:m] if update_sigma2 else None
        nx = None
        if objective_type == "pt2pl":
            if self._target_normals is None:
                raise ValueError("objective_type 'pt2pl' needs target_normals.")
            nx = ph.filter(np.r_[np.zeros((m, y.shape[1])), np.asarray(self._target_normals)], m)[:m]
        return EstepResult(m0, m1, m2, nx)

    def maximization_step(self, t_source, target, estep_res, w=0.0, objective_type="pt2pt"):
        """M-step on explicit E-step arrays (reference filterreg.py:110-113)."""
        return self._maximization_step(t_source, target, estep_res, self._tf_result, self._sigma2, w,
                                       objective_type=objective_type)

    @staticmethod
    @abc.abstractmethod
    def _maximization_step(t_source, target, estep_res, trans_p, sigma2, w=0.0, objective_type="pt2pt"):
        return None

    def registration(self, target, w=0.0, objective_type="pt2pt", maxiter=50, tol=0.001, min_sigma2=1.0e-4,
                     feature_fn=_identity):
        """EM driver (reference filterreg.py:120-147)."""
        assert self._tf_type is not None, "transformation type is None."
        if objective_type not in ("pt2pt", "pt2pl"):
            raise ValueError("Unknown objective_type: %s." % objective_type)
        if objective_type == "pt2pl" and self._target_normals is None:
            raise ValueError("objective_type 'pt2pl' needs target_normals.")
        target = _as_points(target)
        if self._source.shape[1] != target.shape[1] or target.shape[1] not in (2, 3):
            raise ValueError("source and target must both be (n, 2) or (n, 3) arrays.")
        feature_fn = self._resolve_feature_fn(feature_fn)
        if feature_fn is not _identity:
            # any other callable takes the reference's loop (features on the host every iteration)
            return self._registration_features(target, w, objective_type, maxiter, tol, min_sigma2, feature_fn)
        return self._registration_device(target, w, objective_type, maxiter, tol, min_sigma2)

    def _resolve_feature_fn(self, feature_fn):
        """``_identity`` for every spelling of the identity, the callable itself otherwise."""
        if feature_fn is None:  # documented selector of the device-resident path
            feature_fn = _identity
        if feature_fn is not _identity:
            # the reference's own idiom `feature_fn=lambda x: x` (filterreg.py:121): a callable that hands the very
            # object it was given back, UNCHANGED, is the identity - no numerical probe on a sample (an extractor that needs
            # neighbourhoods would misbehave on one), just one call on a COPY of the whole source cloud (an in-place
            # extractor - `x -= x.mean(0); return x` - also returns its argument: it must neither be taken for the
            # identity nor touch the live source)
            probe = self._source.copy()
            if feature_fn(probe) is probe and np.array_equal(probe, self._source):
                feature_fn = _identity
        return feature_fn

    def _registration_device(self, target, w, objective_type, maxiter, tol, min_sigma2):
        """The device-resident loop of the identity ``feature_fn``."""
        dim = target.shape[1]
        q = None
        if self._sigma2 is None:
            self._sigma2 = max(mu.squared_kernel_sum(self._source, target), min_sigma2)
        plan = self._ensure_plan(target)
        plan.set_normals(self._target_normals if objective_type == "pt2pl" else None)
        res = MstepResult(self._tf_result, self._sigma2, None)
        # the transform and sigma2 live on the device: uploaded once, advanced by the M-step kernel
        plan.set_state(self._tf_result.rot, self._tf_result.t, self._sigma2)
        # tf_init_params['scale']: the reference's first transform applies it (filterreg.py:129) and every M-step
        # returns a scale-free RigidTransformation (:196), so it acts on the first iteration only
        scale0 = float(getattr(self._tf_result, "scale", 1.0))
        if scale0 != 1.0:
            plan.set_source(self._source * scale0)
        # Nobody looks at the intermediate results (no callbacks, no tolerance to test, no DEBUG log): the iterations are
        # only enqueued - one lattice-size hand-over per E-step, nothing read back - and the state is fetched once at the
        # end.  An iteration in which every m0 is zero leaves the device state alone (filterreg.py:136-138 would stop there;
        # the iterations after it repeat it and change nothing either).
        if not self._callbacks and tol < 0 and not log.isEnabledFor(10) and scale0 == 1.0 and maxiter > 0:
            for i in range(maxiter):
                plan.estep()
                plan.mstep(w, self._update_sigma2, objective_type, min_sigma2, read=False)
            out = plan.get_state()
            if out[19] > 0.0:
                rot = out[:9].reshape(3, 3)[:dim, :dim].copy()
                res = MstepResult(tf.RigidTransformation(rot, out[9:9 + dim].copy()), float(out[15]), float(out[18]))
                self._tf_result = res.transformation
                self._sigma2 = max(res.sigma2, min_sigma2)
                if out[16] == 0.0:  # the last iterations had nothing to fit: the driver's answer at that point
                    res = MstepResult(self._tf_result, self._sigma2, res.q)
            else:
                res = MstepResult(self._tf_result, self._sigma2, None)
            return res
        for i in range(maxiter):
            if i == 1 and scale0 != 1.0:
                plan.set_source(self._source)
            plan.estep()
            out = plan.mstep(w, self._update_sigma2, objective_type, min_sigma2)
            if out[16] == 0.0:  # every m0 == 0 (filterreg.py:167-168, :136-138)
                res = MstepResult(self._tf_result, self._sigma2, q)
                break
            rot = out[:9].reshape(3, 3)[:dim, :dim].copy()
            t = out[9:9 + dim].copy()
            res = MstepResult(tf.RigidTransformation(rot, t), float(out[15]), float(out[13]))
            self._tf_result = res.transformation
            self._sigma2 = max(res.sigma2, min_sigma2)
            for c in self._callbacks:
                c(self._tf_result)
            log.debug("Iteration: {}, Criteria: {}".format(i, res.q))
            if q is not None and abs(res.q - q) < tol:
                break
            q = res.q
        return res


    def _registration_features(self, target, w, objective_type, maxiter, tol, min_sigma2, feature_fn):
        """The reference's driver verbatim in structure (filterreg.py:120-147) for a non-identity ``feature_fn``:
        features are evaluated on the host every iteration, the lattice E-step and the M-step run on the GPU."""
        q = None
        ftarget = np.asarray(feature_fn(target), dtype=np.float64)
        if self._sigma2 is None:
            fsource = np.asarray(feature_fn(self._source), dtype=np.float64)
            self._sigma2 = max(mu.squared_kernel_sum(fsource, ftarget), min_sigma2)
        res = MstepResult(self._tf_result, self._sigma2, None)
        for i in range(maxiter):
            t_source = self._tf_result.transform(self._source)
            fsource = np.asarray(feature_fn(t_source), dtype=np.float64)
            estep_res = self.expectation_step(fsource, ftarget, target, self._sigma2, self._update_sigma2, objective_type)
            res = self.maximization_step(t_source, target, estep_res, w=w, objective_type=objective_type)
            if res.q is None:
                res = res._replace(q=q)
                break
            self._tf_result = res.transformation
            self._sigma2 = max(res.sigma2, min_sigma2)
            for c in self._callbacks:
                c(self._tf_result)
            log.debug("Iteration: {}, Criteria: {}".format(i, res.q))
            if q is not None and abs(res.q - q) < tol:
                break
            q = res.q
        return res


class RigidFilterReg(FilterReg):
    """Rigid FilterReg (reference filterreg.py:150-196)."""

    def __init__(self, source=None, target_normals=None, sigma2=None, update_sigma2=False, tf_init_params={}):
        super(RigidFilterReg, self).__init__(
            source=source, target_normals=target_normals, sigma2=sigma2, update_sigma2=update_sigma2
        )
        self._tf_type = tf.RigidTransformation
        self._tf_result = self._tf_type(**tf_init_params)
        if self._source is not None and "rot" not in tf_init_params and self._source.shape[1] == 2:
            # the reference needs explicit 2-D tf_init_params for 2-D data (examples/filterreg_rigid2d.py);
            # default to the 2-D identity instead of failing with a shape error
            self._tf_result = self._tf_type(np.identity(2), np.zeros(2))


    @staticmethod
    def _maximization_step(t_source, target, estep_res, trans_p, sigma2, w=0.0, objective_type="pt2pt"):
        """Rigid M-step from explicit arrays (reference filterreg.py:158-196): weighted Kabsch (pt2pt) or twist
        solve (pt2pl) on the GPU, composition with ``trans_p``, sigma2 re-estimated when ``estep_res.m2`` is given."""
        t_source = np.ascontiguousarray(_as_points(t_source))
        target = _as_points(target)
        m, dim = t_source.shape
        assert dim == 2 or dim == 3, "dim must be 2 or 3."
        if objective_type not in ("pt2pt", "pt2pl"):
            raise ValueError("Unknown objective_type: %s." % objective_type)
        m0, m1, m2, nx = estep_res
        if objective_type == "pt2pl" and nx is None:
            raise ValueError("objective_type 'pt2pl' needs estep_res.nx.")
        _lib.require_gpu()
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        m0, m1, m2 = f32(m0), f32(m1), f32(m2)
        nx = f32(nx) if objective_type == "pt2pl" else None
        rot = np.identity(3)
        rot[:dim, :dim] = trans_p.rot
        t = np.zeros(3)
        t[:dim] = trans_p.t
        dev, st = _current_device_and_stream()
        out = np.zeros(18)
        check(lib.prg_fr_mstep_from_arrays(dev, ctypes.c_void_p(st), ptr(t_source), m, dim, target.shape[0], ptr(m0),
                                           ptr(m1), ptr(m2), ptr(nx), ptr(np.ascontiguousarray(rot)), ptr(t),
                                           float(sigma2), float(w), ptr(out)))
        if out[16] == 0.0:  # every m0 == 0 (filterreg.py:167-168)
            return MstepResult(trans_p, sigma2, None)
        return MstepResult(tf.RigidTransformation(out[:9].reshape(3, 3)[:dim, :dim].copy(), out[9:9 + dim].copy()),
                           float(out[15]), float(out[13]))


def _moment_block(mom):
    """sum s^2 J^T J, J = [-[x]x | I] (se3_op.py:56-59), from the ten sums s^2 (1, x, y, z, xx, xy, xz, yy, yz, zz)."""
    n, x, y, z, xx, xy, xz, yy, yz, zz = mom
    blk = np.zeros((6, 6))
    blk[:3, :3] = [[yy + zz, -xy, -xz], [-xy, xx + zz, -yz], [-xz, -yz, xx + yy]]
    blk[:3, 3:] = [[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]]
    blk[3:, :3] = blk[:3, 3:].T
    blk[3:, 3:] = n * np.identity(3)
    return blk


def _assemble_normal(seg_a, seg_b, sums, k, reference_form):
    """The 6K x 6K normal matrix from the per-segment device sums, segments in ascending key order."""
    a = np.zeros((6 * k, 6 * k))
    for na, nb, row in zip(seg_a, seg_b, sums):
        ia, ib = slice(6 * na, 6 * na + 6), slice(6 * nb, 6 * nb + 6)
        cross = _moment_block(row[10:20])
        if reference_form:  # filterreg.py:228-236: off-diagonal node blocks only, ordered pairs of different nodes
            if na != nb:
                a[ia, ib] += cross
                a[ib, ia] += cross
        else:
            a[ia, ia] += _moment_block(row[0:10])
            a[ia, ib] += cross
            a[ib, ia] += cross
            a[ib, ib] += _moment_block(row[20:30])
    return a


def _assemble_gradient(seg_a, seg_b, sums, k, reference_form):
    """(b, q) from the per-segment gradient sums."""
    b = np.zeros(6 * k)
    for na, nb, row in zip(seg_a, seg_b, sums):
        if reference_form:  # filterreg.py:247-254: into the first node of the pair only
            if na != nb:
                b[6 * na:6 * na + 6] += row[0:6]
        else:
            b[6 * na:6 * na + 6] += row[0:6]
            b[6 * nb:6 * nb + 6] += row[6:12]
    return b, float(np.sum(sums[:, 12]))


def _kinematic_weights(weights, m):
    """(pairs int32 (m, 2), vals float32 (m, 2), K) of a SkinningWeight, checked."""
    if weights is None:
        raise ValueError("skinning weights are needed.")
    pairs = np.ascontiguousarray(weights["pair"], dtype=np.int32).reshape(-1, 2)
    vals = np.ascontiguousarray(weights["val"], dtype=np.float32).reshape(-1, 2)
    if pairs.shape[0] != m:
        raise ValueError("%d skinning weights for %d source points." % (pairs.shape[0], m))
    return pairs, vals


def _kinematic_solve(plan, dualquats, sigma2, w, update_sigma2, maxiter, tol, reference_form):
    """The M-step of DESIGN.md section 3.10 on a plan that holds E-step values: normal sums once, then the Gauss-Newton
    inner loop - per iteration 6K increments go to the device and the per-segment gradient sums come back.
    Returns (dualquats, sigma2, q, inner iterations); q None when no point has m0 != 0."""
    k = plan.n_nodes
    nsum = plan.kinematic_normal_sums(sigma2, w, reference_form)
    if float(np.sum(nsum[:, 32])) == 0.0:
        return dualquats, sigma2, None, 0
    a = _assemble_normal(plan.seg_a, plan.seg_b, nsum, k, reference_form)
    # minimum-norm least squares with the cut-off of np.linalg.lstsq(rcond=None), factored once: A is constant over the loop
    pinv = np.linalg.pinv(a, rcond=np.finfo(np.float64).eps * a.shape[0])
    tw = np.zeros(6 * k)
    q, n_iter = None, 0
    for _ in range(maxiter):
        b, q = _assemble_gradient(plan.seg_a, plan.seg_b, plan.kinematic_grad_sums(tw, reference_form), k, reference_form)
        dtw = pinv @ b
        tw -= dtw
        n_iter += 1
        if np.linalg.norm(dtw) < tol:
            break
    used = np.zeros(k, dtype=bool)
    used[plan.seg_a] = used[plan.seg_b] = True  # (a node that no point names keeps its dual quaternion as it is)
    new = np.array([tf.dualquat_mul(tf.dualquat_from_twist(tw[6 * i:6 * i + 6]), dualquats[i]) if used[i]
                    else np.asarray(dualquats[i], dtype=np.float64) for i in range(k)])
    if update_sigma2:  # filterreg.py:263-264
        sigma2 = float(np.sum(nsum[:, 30])) / (3.0 * float(np.sum(nsum[:, 31])))
    return new, sigma2, q, n_iter


class DeformableKinematicFilterReg(FilterReg):
    """FilterReg with the deformable kinematic model (reference filterreg.py:199-266): the source moves by
    dual-quaternion skinning of ``skinning_weight.n_nodes`` nodes, two per point.

    source          : (M, 3) array
    skinning_weight : ``transformation.DeformableKinematicModel.SkinningWeight`` of length M
    sigma2          : kernel variance (None = automatic)
    update_sigma2   : re-estimate sigma2 in every M-step (an extension: the reference never does here)

    With the identity ``feature_fn`` the EM loop stays on the device (skinning, lattice E-step, M-step sums); any other
    callable takes the driver of the base class.  The M-step is the complete Gauss-Newton system of DESIGN.md section
    3.10; ``_maximization_step(..., reference_form=True)`` is the reference's own.  The result's transformation carries
    ``inner_iterations``, the Gauss-Newton iterations of the last M-step.
    """

    def __init__(self, source=None, skinning_weight=None, sigma2=None, update_sigma2=False):
        super(DeformableKinematicFilterReg, self).__init__(source, sigma2=sigma2, update_sigma2=update_sigma2)
        if skinning_weight is None:
            raise ValueError("DeformableKinematicFilterReg needs skinning weights.")
        self._tf_type = tf.DeformableKinematicModel
        self._skinning_weight = skinning_weight
        if self._source is not None:
            self._check_source()
        self._tf_result = self._tf_type(tf.dualquat_identity(self._skinning_weight.n_nodes), self._skinning_weight)

    def _check_source(self):
        if self._source.ndim != 2 or self._source.shape[1] != 3:
            raise ValueError("dim must be 3.")  # filterreg.py:219
        _kinematic_weights(self._skinning_weight, self._source.shape[0])
        if int(np.min(self._skinning_weight["pair"])) < 0:
            raise ValueError("skinning weights name a node outside [0, %d)." % self._skinning_weight.n_nodes)

    def set_source(self, source):
        super(DeformableKinematicFilterReg, self).set_source(source)
        self._check_source()

    @staticmethod
    def _maximization_step(t_source, target, estep_res, trans_p, sigma2, w=0.0, objective_type="", maxiter=50, tol=1.0e-4,
                           reference_form=False):
        """Kinematic M-step from explicit arrays (reference filterreg.py:211-266).  The arrays go
        to the device once; the inner loop exchanges increments and per-segment sums only.  sigma2 is re-estimated
        when ``estep_res.m2`` is given."""
        t_source = np.ascontiguousarray(_as_points(t_source))
        target = _as_points(target)
        if t_source.ndim != 2 or t_source.shape[1] != 3:
            raise ValueError("dim must be 3.")
        m = t_source.shape[0]
        m0, m1, m2 = estep_res[0], estep_res[1], estep_res[2]
        pairs, vals = _kinematic_weights(trans_p.weights, m)
        dualquats = np.asarray(trans_p.dualquats, dtype=np.float64).reshape(-1, 8)
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        plan = _Plan()
        try:
            plan.set_source(t_source)
            plan.set_skinning(pairs, vals, dualquats.shape[0])
            plan.kinematic_set_arrays(t_source, f32(m0), f32(m1), f32(m2), target.shape[0])
            dq, sigma2_new, q, n_iter = _kinematic_solve(plan, dualquats, sigma2, w, m2 is not None, maxiter, tol,
                                                        reference_form)
        finally:
            plan.close()
        if q is None:
            return MstepResult(trans_p, sigma2, None)
        model = tf.DeformableKinematicModel(dq, trans_p.weights)
        model.inner_iterations = n_iter
        return MstepResult(model, sigma2_new, q)

    def _registration_device(self, target, w, objective_type, maxiter, tol, min_sigma2):
        """filterreg.py:120-147 with everything per point on the device: the source is skinned there, the lattice
        E-step leaves m0, m1, m2 there and the M-step sums read them in place."""
        if target.shape[1] != 3:
            raise ValueError("dim must be 3.")
        self._check_source()
        q = None
        if self._sigma2 is None:
            self._sigma2 = max(mu.squared_kernel_sum(self._source, target), min_sigma2)
        plan = self._ensure_plan(target)
        pairs, vals = _kinematic_weights(self._skinning_weight, self._source.shape[0])
        plan.set_skinning(pairs, vals, self._tf_result.dualquats.shape[0])
        res = MstepResult(self._tf_result, self._sigma2, None)
        for i in range(maxiter):
            plan.set_dualquats(self._tf_result.dualquats)
            plan.kinematic_estep(self._sigma2)
            dq, sigma2, qn, n_iter = _kinematic_solve(plan, self._tf_result.dualquats, self._sigma2, w, self._update_sigma2,
                                                     50, 1.0e-4, False)
            if qn is None:  # every m0 == 0 (filterreg.py:136-138)
                res = MstepResult(self._tf_result, self._sigma2, q)
                break
            model = tf.DeformableKinematicModel(dq, self._skinning_weight)
            model.inner_iterations = n_iter
            res = MstepResult(model, sigma2, qn)
            self._tf_result = res.transformation
            self._sigma2 = max(res.sigma2, min_sigma2)
            for c in self._callbacks:
                c(self._tf_result)
            log.debug("Iteration: {}, Criteria: {}".format(i, res.q))
            if q is not None and abs(res.q - q) < tol:
                break
            q = res.q
        return res


def kinematic_system(t_source, target_count, estep_res, weights, sigma2, w=0.0, reference_form=False):
    """(A, b) of the kinematic M-step from the device sums: the 6K x 6K normal matrix and the
    gradient at zero increments.  ``weights`` is a SkinningWeight, ``estep_res`` an EstepResult (or (m0, m1, ...))."""
    t_source = np.ascontiguousarray(_as_points(t_source))
    if t_source.ndim != 2 or t_source.shape[1] != 3:
        raise ValueError("dim must be 3.")
    m = t_source.shape[0]
    pairs, vals = _kinematic_weights(weights, m)
    k = int(pairs.max()) + 1
    _lib.require_gpu()
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    m0, m1 = f32(estep_res[0]), f32(estep_res[1])
    m2 = f32(estep_res[2]) if len(estep_res) > 2 else None
    keys = np.unique(pairs[:, 0].astype(np.int64) * k + pairs[:, 1])
    seg_a, seg_b = keys // k, keys % k
    nsum, gsum = np.empty((keys.shape[0], 34)), np.empty((keys.shape[0], 16))
    dev, st = _current_device_and_stream()
    check(lib.prg_fr_kinematic_sums_from_arrays(dev, ctypes.c_void_p(st), ptr(t_source), m, int(target_count), ptr(m0),
                                                ptr(m1), None if m2 is None else ptr(m2), ptr(pairs), ptr(vals), k,
                                                float(sigma2), float(w), 1 if reference_form else 0, None,
                                                keys.shape[0], ptr(nsum), ptr(gsum)))
    return (_assemble_normal(seg_a, seg_b, nsum, k, reference_form),
            _assemble_gradient(seg_a, seg_b, gsum, k, reference_form)[0])


def registration_filterreg(source, target, target_normals=None, sigma2=None, update_sigma2=False, w=0,
                           objective_type="pt2pt", maxiter=50, tol=0.001, min_sigma2=1.0e-4, feature_fn=_identity,
                           callbacks=[], **kwargs):
    """One-call rigid FilterReg with the reference's signature (filterreg.py:269-317).

    source, target  : (n, 2|3) arrays or Open3D point clouds
    target_normals  : (N, 3) normals, required for ``objective_type='pt2pl'``
    sigma2          : kernel variance (None = automatic); update_sigma2 re-estimates it every iteration
    w               : outlier mass in [0, 1); objective_type 'pt2pt' (Kabsch) or 'pt2pl' (twist)
    maxiter, tol    : stop after maxiter iterations or when |q - q_prev| < tol; min_sigma2 clamps the variance
    feature_fn      : maps (n, D) points to (n, d <= 64) features the lattice is built over (identity by default; a
                      host callable, evaluated once per iteration); callbacks get the transformation after every iteration
    **kwargs        : ``tf_init_params`` for the starting rigid transform
    Returns ``MstepResult(transformation, sigma2, q)``.
    """
    frg = RigidFilterReg(_as_points(source), _as_points(target_normals), sigma2, update_sigma2, **kwargs)
    frg.set_callbacks(callbacks)
    return frg.registration(
        _as_points(target), w=w, objective_type=objective_type, maxiter=maxiter, tol=tol, min_sigma2=min_sigma2,
        feature_fn=feature_fn,
    )


def kabsch(model, target, weight):
    """Weighted Kabsch on the GPU (reference ``_kabsch.kabsch`` / ``kabsch2d``, cc/kabsch.cc:6-109)."""
    _lib.require_gpu()
    model = np.ascontiguousarray(model, dtype=np.float32)
    target = np.ascontiguousarray(target, dtype=np.float32)
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    dim = model.shape[1]
    dev, st = _current_device_and_stream()
    rot = np.empty((dim, dim))
    t = np.empty(dim)
    check(lib.prg_kabsch_weighted(dev, ctypes.c_void_p(st), ptr(model), ptr(target), ptr(weight), model.shape[0], dim,
                                  ptr(rot), ptr(t)))
    return rot, t
