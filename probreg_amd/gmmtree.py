"""GMMTree registration on MI355X - drop-in for ``probreg.gmmtree`` (reference probreg/gmmtree.py, cc/gmmtree.{h,cc}).

Public surface as in the reference: ``EstepResult`` / ``MstepResult`` (gmmtree.py:13-14), ``GMMTree`` (:23-96),
``registration_gmmtree`` (:99-129).  The algorithm is Eckart et al., "HGMR: Hierarchical Gaussian Mixtures for Adaptive
3D Registration", ECCV 2018.

What runs where
  * Tree build (``buildGmmTree`` gmmtree.cc:98-123): EM level by level in ``libprobreg_hip.so`` (``prg_gmm_build``).
    One fp64 log-likelihood crosses to the host per EM iteration for the reference's stop test ``|q - q_prev| < lambda_s``.
  * Registration E-step (``gmmTreeRegEstep`` :175-214): transform, tree descent and the per-node moments on the GPU, the
    target resident there across iterations (``prg_gmm_reg_estep``); only ``(m0, m1)`` per node is read back.
  * M-step (gmmtree.py:64-81): the reference's own algebra on the host, vectorised - the eigen-decompositions of all
    node covariances once per tree (batched ``np.linalg.eigh``), the ``3 n_nodes x 6`` system from array operations and
    the reference's ``np.linalg.lstsq(amat, bmat, rcond=-1)``, so ``q`` is lstsq's residual array (shape ``(0,)`` when
    the rank is below 6, and the stop test then raises ``ValueError`` under NumPy >= 2.2 exactly like the reference).

Differences a caller can see (all on purpose):
  * Precision: the whole tree path (node parameters, Gaussians, reductions, ``q``, M-step) is fp64; the reference's
    native code is float (cc/types.h:5).  Results are reproducible: same inputs on the same device give byte-identical
    trees, moments and registrations (fixed-order reductions, no floating-point atomics).
  * Initialisation: leaf ``k`` of the tree starts at point ``idx[k]`` (mean and the covariance about it) with
    ``idx = np.random.default_rng(seed).integers(0, N, 8**tree_level)``; the reference draws from an unseeded
    ``std::rand`` and cannot be reproduced.
  * Keyword-only extensions: ``seed=0``; ``max_build_iter`` (per-level EM cap, default 1000; the reference has none -
    a warning is logged when it is hit); ``device``.  ``nodes`` (also as ``_nodes``) is a read-only host view of the tree
    in the reference's ``(pi, mu, Sigma)`` tuple format and ``set_nodes(nodes)`` installs a given tree without a build.
  * ``1 <= tree_level <= 4`` (4 680 nodes); other levels raise ``ValueError``.  3-D clouds only, as the reference.

With ``torch.distributed`` initialised every rank solves the whole problem (replicas; nothing is sharded).  Work runs on
the caller's current HIP stream.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from . import transformation as tf
from ._lib import as_points as _as_points
from .log import log

EstepResult = namedtuple("EstepResult", ["moments"])
MstepResult = namedtuple("MstepResult", ["transformation", "q"])
MstepResult.__doc__ = """Result of the M-step (reference gmmtree.py:14): the RigidTransformation and q, the residual array
    of the least-squares solve."""

N_NODE = 8
MAX_TREE_LEVEL = 4
LAMBDA_D = 1.0e-4  # gmmtree.py:51
DEFAULT_MAX_BUILD_ITER = 1000


def n_nodes(tree_level):
    """Nodes of a tree of ``tree_level`` levels: 8 (8^L - 1) / 7 (gmmtree.cc:44)."""
    return N_NODE * (N_NODE ** tree_level - 1) // (N_NODE - 1)


def init_indices(n_points, tree_level, seed=0):
    """Points the leaves start from (the deterministic counterpart of gmmtree.cc:47)."""
    return np.random.default_rng(seed).integers(0, n_points, N_NODE ** tree_level).astype(np.int64)


# ---- se3_op (reference se3_op.py:20-53) -----------------------------------------------------------------------------
def skew(x):
    return np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])


def twist_trans(tw, linear=False):
    """Twist -> (rotation, translation) (se3_op.py:20-41, Rodrigues)."""
    if linear:
        return np.identity(3) + skew(tw[:3]), tw[3:]
    twd = np.linalg.norm(tw[:3])
    if twd == 0.0:
        return np.identity(3), tw[3:]
    ntw = tw[:3] / twd
    c = np.cos(twd)
    s = np.sin(twd)
    tr = c * np.identity(3) + (1.0 - c) * np.outer(ntw, ntw) + s * skew(ntw)
    return tr, tw[3:]


def twist_mul(tw, rot, t, linear=False):
    """Apply a twist to (rot, t) (se3_op.py:44-53)."""
    tr, tt = twist_trans(tw, linear=linear)
    return np.dot(tr, rot), np.dot(t, tr.T) + tt


# ---- node records -----------------------------------------------------------------------------------------------------
_SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
_UPPER = (np.array([0, 0, 0, 1, 1, 2]), np.array([0, 1, 2, 1, 2, 2]))


def nodes_to_array(nodes):
    """Reference ``_nodes`` (sequence of (pi, mu (3,), Sigma (3, 3))) -> (n, 10) float64 records."""
    if isinstance(nodes, np.ndarray) and nodes.ndim == 2 and nodes.shape[1] == 10:
        return np.ascontiguousarray(nodes, dtype=np.float64)
    out = np.empty((len(nodes), 10))
    for j, (pi, mu, sig) in enumerate(nodes):
        sig = np.asarray(sig, dtype=np.float64)
        out[j, 0] = pi
        out[j, 1:4] = mu
        out[j, 4:] = sig[_UPPER]
    return out


def array_to_nodes(arr):
    """(n, 10) records -> tuple of (pi, mu, Sigma) with read-only arrays (the reference's ``_nodes`` format)."""
    mu = arr[:, 1:4].copy()
    sig = arr[:, 4:][:, _SYM]
    mu.flags.writeable = False
    sig.flags.writeable = False
    return tuple((float(arr[j, 0]), mu[j], sig[j]) for j in range(arr.shape[0]))


def _tree_level_of(count):
    for lv in range(1, MAX_TREE_LEVEL + 1):
        if n_nodes(lv) == count:
            return lv
    raise ValueError("a GMM tree has 8 (8^L - 1) / 7 nodes for 1 <= L <= %d, not %d" % (MAX_TREE_LEVEL, count))


class GmmTreePlan(_lib.Handle):
    """One ``prg_gmmtree`` handle: the tree and the registration target on one device / stream."""

    def __init__(self, device=None):
        super().__init__(_lib.lib.prg_gmm_create, _lib.lib.prg_gmm_destroy, device)
        self.tree_level = 0

    def build(self, points, tree_level, idx, lambda_s, lambda_d, max_iter):
        pts = np.ascontiguousarray(points, dtype=np.float64)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        iters = np.zeros(tree_level, dtype=np.int32)
        q = np.zeros(tree_level)
        dq = np.zeros(tree_level)
        _lib.check(_lib.lib.prg_gmm_build(self._h, _lib.ptr(pts), pts.shape[0], int(tree_level), _lib.ptr(idx),
                                          float(lambda_s), float(lambda_d), int(max_iter), _lib.ptr(iters), _lib.ptr(q),
                                          _lib.ptr(dq)))
        self.tree_level = int(tree_level)
        return iters, q, dq

    def set_nodes(self, arr, tree_level):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        _lib.check(_lib.lib.prg_gmm_set_nodes(self._h, _lib.ptr(arr), int(tree_level)))
        self.tree_level = int(tree_level)

    def get_nodes(self):
        out = np.empty((n_nodes(self.tree_level), 10))
        _lib.check(_lib.lib.prg_gmm_get_nodes(self._h, _lib.ptr(out)))
        return out

    def set_target(self, target):
        tgt = np.ascontiguousarray(target, dtype=np.float64)
        _lib.check(_lib.lib.prg_gmm_set_target(self._h, _lib.ptr(tgt), tgt.shape[0]))

    def reg_estep(self, rot, t, scale, lambda_c, with_m2=False):
        """(m01 (n_nodes, 4), m2 (n_nodes, 6) or None) for the target moved by scale * rot + t."""
        rot = np.ascontiguousarray(rot, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        nn = n_nodes(self.tree_level)
        m01 = np.empty((nn, 4))
        m2 = np.empty((nn, 6)) if with_m2 else None
        _lib.check(_lib.lib.prg_gmm_reg_estep(self._h, _lib.ptr(rot), _lib.ptr(t), float(scale), float(lambda_c),
                                              _lib.ptr(m01), _lib.ptr(m2)))
        return m01, m2


def _check_level(tree_level):
    if not (isinstance(tree_level, (int, np.integer)) and 1 <= int(tree_level) <= MAX_TREE_LEVEL):
        raise ValueError("tree_level must be an integer in [1, %d], got %r" % (MAX_TREE_LEVEL, tree_level))
    return int(tree_level)


def _check_cloud(x, what):
    x = _as_points(x)
    if x.ndim != 2 or x.shape[1] != 3 or x.shape[0] < 1:
        raise ValueError("%s must be a non-empty (n, 3) array, got shape %s" % (what, x.shape))
    return x


class GMMTree(object):
    """GMM tree registration (reference gmmtree.py:23-96).

    Args:
        source: source cloud (n, 3) or Open3D point cloud; the tree is built from it.
        tree_level: depth of the tree, 1..4.
        lambda_c: pruning threshold of the registration E-step's descent (complexity <= lambda_c stops it).
        lambda_s: stop tolerance of each level's EM in the build.
        tf_init_params: keyword arguments of the initial ``RigidTransformation``.
    Keyword-only extensions: ``seed`` (leaf initialisation), ``max_build_iter`` (EM cap per level), ``device``.
    """

    def __init__(self, source=None, tree_level=2, lambda_c=0.01, lambda_s=0.001, tf_init_params={}, *, seed=0,
                 max_build_iter=DEFAULT_MAX_BUILD_ITER, device=None):
        self._tree_level = _check_level(tree_level)
        self._lambda_c = lambda_c
        self._lambda_s = lambda_s
        self._seed = seed
        self._max_build_iter = int(max_build_iter)
        self._device = device
        self._tf_type = tf.RigidTransformation
        self._tf_result = self._tf_type(**tf_init_params)
        self._callbacks = []
        self._plan = None
        self._tree = None
        self._eig = None
        self._target_id = None
        self.build_iterations = None
        self.build_q = None
        self._source = None
        if source is not None:
            self.set_source(source)

    # -- tree ---------------------------------------------------------------------------------------------------------
    def _ensure_plan(self):
        if self._plan is None:
            self._plan = GmmTreePlan(self._device)
        return self._plan

    def close(self):
        if self._plan is not None:
            self._plan.close()
            self._plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def set_source(self, source):
        """Build the tree from ``source`` (gmmtree.py:55-57 -> buildGmmTree gmmtree.cc:98-123)."""
        self._source = _check_cloud(source, "source")
        plan = self._ensure_plan()
        idx = init_indices(self._source.shape[0], self._tree_level, self._seed)
        iters, q, _ = plan.build(self._source, self._tree_level, idx, self._lambda_s, LAMBDA_D, self._max_build_iter)
        for lv in range(self._tree_level):
            if iters[lv] >= self._max_build_iter:
                log.warning("GMMTree build: level %d stopped at max_build_iter=%d before |dq| < lambda_s=%g",
                            lv, self._max_build_iter, self._lambda_s)
        self.build_iterations = iters
        self.build_q = q
        self._set_tree(plan.get_nodes())
        self._target_id = None

    def set_nodes(self, nodes):
        """Install a given tree (reference ``_nodes`` format or (n, 10) records) instead of building one."""
        arr = nodes_to_array(nodes)
        self._tree_level = _tree_level_of(arr.shape[0])
        self._ensure_plan().set_nodes(arr, self._tree_level)
        self._set_tree(arr)
        self._target_id = None

    def _set_tree(self, arr):
        self._tree = np.ascontiguousarray(arr)
        self._tree.flags.writeable = False
        self._nodes_view = None
        self._eig = None

    @property
    def nodes(self):
        """Read-only host view of the tree: tuple of (pi, mu (3,), Sigma (3, 3)) (the reference's ``_nodes``)."""
        if self._tree is None:
            return None
        if self._nodes_view is None:
            self._nodes_view = array_to_nodes(self._tree)
        return self._nodes_view

    _nodes = nodes

    def set_callbacks(self, callbacks):
        self._callbacks = callbacks

    # -- EM -----------------------------------------------------------------------------------------------------------
    def _require_tree(self):
        if self._tree is None:
            raise RuntimeError("GMMTree: no tree - pass a source or call set_source / set_nodes first")

    def expectation_step(self, target):
        """gmmTreeRegEstep on an already transformed target (gmmtree.py:59-61): moments as a list of
        (m0, m1 (3,), m2 (3, 3)) per node."""
        self._require_tree()
        target = _check_cloud(target, "target")
        plan = self._plan
        plan.set_target(target)
        self._target_id = None
        m01, m2 = plan.reg_estep(np.identity(3), np.zeros(3), 1.0, self._lambda_c, with_m2=True)
        m2f = m2[:, _SYM]
        return EstepResult([(float(m01[j, 0]), m01[j, 1:4].copy(), m2f[j]) for j in range(m01.shape[0])])

    def _eigh(self):
        if self._eig is None:
            sig = self._tree[:, 4:][:, _SYM]
            self._eig = np.linalg.eigh(sig)
        return self._eig

    def _mstep(self, m0, m1, trans_p):
        """gmmtree.py:64-81 on all nodes at once."""
        n = m0.shape[0]
        lmd, nn = self._eigh()
        use = m0 >= np.finfo(np.float32).eps
        amat = np.zeros((n, 3, 6))
        bmat = np.zeros((n, 3))
        if np.any(use):
            mu = self._tree[use, 1:4]
            s = m1[use] / m0[use][:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                nns = nn[use] * np.sqrt(m0[use][:, None] / lmd[use])[:, None, :]
            rows = np.swapaxes(nns, 1, 2)  # nn.T per node: row k = eigenvector k scaled
            bmat[use] = np.einsum("nkd,nd->nk", rows, mu) - np.einsum("nkd,nd->nk", rows, s)
            amat[use, :, :3] = np.cross(s[:, None, :], rows)
            amat[use, :, 3:] = rows
        x, q, _, _ = np.linalg.lstsq(amat.reshape(3 * n, 6), bmat.reshape(3 * n), rcond=-1)
        rot, t = twist_mul(x, trans_p.rot, trans_p.t)
        return MstepResult(tf.RigidTransformation(rot, t), q)

    def maximization_step(self, estep_res, trans_p):
        """gmmtree.py:63-81.  ``estep_res.moments``: the list of ``expectation_step`` or an (n_nodes, >= 4) array whose
        first columns are (m0, m1)."""
        self._require_tree()
        mom = estep_res.moments
        if isinstance(mom, np.ndarray):
            m0 = np.asarray(mom[:, 0], dtype=np.float64)
            m1 = np.asarray(mom[:, 1:4], dtype=np.float64)
        else:
            m0 = np.array([float(m[0]) for m in mom])
            m1 = np.array([np.asarray(m[1], dtype=np.float64) for m in mom]).reshape(-1, 3)
        if m0.shape[0] != self._tree.shape[0]:
            raise ValueError("moments for %d nodes, the tree has %d" % (m0.shape[0], self._tree.shape[0]))
        return self._mstep(m0, m1, trans_p)

    def registration(self, target, maxiter=20, tol=1.0e-4):
        """EM loop of the reference (gmmtree.py:83-96) with the target resident on the GPU."""
        self._require_tree()
        target = _check_cloud(target, "target")
        plan = self._plan
        plan.set_target(target)
        q = None
        res = None
        for i in range(maxiter):
            tfr = self._tf_result
            m01, _ = plan.reg_estep(tfr.rot, tfr.t, tfr.scale, self._lambda_c)  # transform + E-step (:87-88)
            res = self._mstep(m01[:, 0], m01[:, 1:4], tfr)
            self._tf_result = res.transformation
            for c in self._callbacks:
                c(self._tf_result.inverse())
            log.debug("Iteration: {}, Criteria: {}".format(i, res.q))
            if q is not None and abs(res.q - q) < tol:
                break
            q = res.q
        self.iterations = i + 1 if maxiter > 0 else 0
        return MstepResult(self._tf_result.inverse(), res.q if res is not None else None)


def registration_gmmtree(source, target, maxiter=20, tol=1.0e-4, callbacks=[], **kwargs):
    """One-call GMMTree registration with the reference's signature (gmmtree.py:99-129).

    source, target : (n, 3) arrays or Open3D point clouds
    maxiter, tol   : EM iterations, stop when the least-squares residual changes by < tol
    callbacks      : called after each iteration with the current source -> target estimate
    **kwargs       : ``tree_level``, ``lambda_c``, ``lambda_s``, ``tf_init_params`` of :class:`GMMTree`, and the
                     keyword-only extensions ``seed``, ``max_build_iter``, ``device``
    Returns MstepResult(transformation, q).
    """
    gt = GMMTree(_as_points(source), **kwargs)
    gt.set_callbacks(callbacks)
    try:
        return gt.registration(_as_points(target), maxiter, tol)
    finally:
        gt.close()
