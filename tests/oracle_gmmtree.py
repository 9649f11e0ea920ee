"""fp64 NumPy restatement of the reference's GMMTree native code (TEST INFRASTRUCTURE).

Restates probreg/cc/gmmtree.cc (the reference's ``probreg._gmmtree``) vectorised over points, in float64 (the reference
is float, cc/types.h:5; the product is fp64 on the device):
  ``init_nodes``  initializeNodes :46-73 with explicit leaf indices (the reference draws them from std::rand)
  ``build``       buildGmmTree :98-123 (gmmTreeEstep :125-163, gmmTreeMstep / mlEstimator :165-173 / :81-96,
                  logLikelihood :20-33) with an iteration cap per level
  ``reg_estep``   gmmTreeRegEstep :175-214
``OracleGmmTreePlan`` is a stand-in for ``probreg_amd.gmmtree.GmmTreePlan`` so the product's Python driver runs without a
GPU; ``standin_module`` is a stand-in for the pybind module ``probreg._gmmtree`` under the unmodified reference driver.
It is never imported by the product.
"""
import types

import numpy as np

N_NODE = 8
EPS = 1.0e-15            # gmmtree.cc:9
TWO_PI_15 = (2.0 * np.pi) ** 1.5
SYM = np.array([[0, 1, 2], [1, 3, 4], [2, 4, 5]])
UPPER = (np.array([0, 0, 0, 1, 1, 2]), np.array([0, 1, 2, 1, 2, 2]))
BLOCK = 1 << 22          # point x node pairs per vectorised block


def level(l):
    """First node of level l (gmmtree.cc:44)."""
    return N_NODE * (N_NODE ** l - 1) // (N_NODE - 1)


def n_nodes(tree_level):
    return level(tree_level)


def init_indices(n_points, tree_level, seed=0):
    return np.random.default_rng(seed).integers(0, n_points, N_NODE ** tree_level).astype(np.int64)


def init_nodes(points, tree_level, idx):
    """initializeNodes (gmmtree.cc:46-73): (n_nodes, 10) records (pi, mu, Sigma upper xx xy xz yy yz zz)."""
    p = np.asarray(points, dtype=np.float64)
    nodes = np.zeros((n_nodes(tree_level), 10))
    m = p.mean(axis=0)
    d = p - m
    cov = d.T @ d / p.shape[0]
    lf = level(tree_level - 1)
    for j, k in enumerate(idx):  # Sigma = sum_i (p_i - p_k)(p_i - p_k)^T / N = C + (m - p_k)(m - p_k)^T
        e = m - p[k]
        sig = cov + np.outer(e, e)
        nodes[lf + j, 0] = 1.0 / N_NODE
        nodes[lf + j, 1:4] = p[k]
        nodes[lf + j, 4:] = sig[UPPER]
    for l in range(tree_level - 2, -1, -1):  # :55-72 moment matching of the 8 children
        pidx, cidx = level(l), level(l + 1)
        for j in range(N_NODE ** (l + 1)):
            ch = nodes[cidx + j * N_NODE: cidx + (j + 1) * N_NODE]
            cm = ch[:, 1:4]
            csig = ch[:, 4:][:, SYM]
            mu = cm.mean(axis=0)
            sig = (csig + cm[:, :, None] * cm[:, None, :]).mean(axis=0) - np.outer(mu, mu)
            nodes[pidx + j, 0] = 1.0 / N_NODE
            nodes[pidx + j, 1:4] = mu
            nodes[pidx + j, 4:] = sig[UPPER]
    return nodes


def precompute(nodes):
    """Per node: pi * c (0 when det < eps, gaussianPdf :11-18), Sigma^-1 (0 there) and complexity (:35-40)."""
    sig = nodes[:, 4:][:, SYM]
    det = np.linalg.det(sig)
    live = det >= EPS
    pic = np.zeros(nodes.shape[0])
    pic[live] = nodes[live, 0] / (np.sqrt(det[live]) * TWO_PI_15)
    inv = np.zeros_like(sig)
    if np.any(live):
        inv[live] = np.linalg.inv(sig[live])
    lmd = np.linalg.eigvalsh(sig)
    with np.errstate(divide="ignore", invalid="ignore"):
        cplx = lmd[:, 0] / lmd.sum(axis=1)
    return pic, inv, cplx


def _weighted_pdf(x, mu, inv, pic):
    """pi_j pdf_j(x_i) for per-point node parameters (leading axes broadcast): x (..., 3), mu (..., 3), inv (..., 3, 3)."""
    d = x - mu
    q = np.einsum("...d,...de,...e->...", d, inv, d)
    with np.errstate(over="ignore", under="ignore"):
        return np.where(pic == 0.0, 0.0, pic * np.exp(-0.5 * q))


def _normalise(g):
    den = g.sum(axis=1)
    ok = den > EPS
    out = np.zeros_like(g)
    out[ok] = g[ok] / den[ok, None]
    return out


def _top2_gap(g):
    if g.shape[0] == 0:
        return np.inf
    s = np.sort(g, axis=1)
    live = s[:, -1] > 0.0
    return float(np.min(s[live, -1] - s[live, -2])) if np.any(live) else np.inf


def build_estep(points, nodes, pre, parent):
    """gmmTreeEstep (:125-163): moments (m0 (n,), m1 (n, 3), m2 (n, 3, 3)) over all nodes, `current`, min top-two gap."""
    pic, inv, _ = pre
    n = nodes.shape[0]
    m0, m1, m2 = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3, 3))
    cur = np.empty(points.shape[0], dtype=np.int64)
    gap = np.inf
    step = max(1, BLOCK // N_NODE)
    for a in range(0, points.shape[0], step):
        x = points[a:a + step]
        j = (parent[a:a + step, None] + 1) * N_NODE + np.arange(N_NODE)[None, :]
        g = _normalise(_weighted_pdf(x[:, None, :], nodes[j, 1:4], inv[j], pic[j]))
        cur[a:a + step] = j[np.arange(x.shape[0]), np.argmax(g, axis=1)]  # first maximum, as Eigen's maxCoeff
        gap = min(gap, _top2_gap(g))
        jf, gf = j.ravel(), g.ravel()
        xr = np.repeat(x, N_NODE, axis=0)
        m0 += np.bincount(jf, gf, minlength=n)
        for k in range(3):
            m1[:, k] += np.bincount(jf, gf * xr[:, k], minlength=n)
            for l2 in range(3):
                m2[:, k, l2] += np.bincount(jf, gf * xr[:, k] * xr[:, l2], minlength=n)
    return (m0, m1, m2), cur, gap


def ml_estimator(m0, m1, m2, n_points, lambda_d):
    """mlEstimator (:81-96) for a set of nodes -> (k, 10) records."""
    out = np.zeros((m0.shape[0], 10))
    out[:, 0] = m0 / n_points
    dead = m0 < lambda_d
    live = ~dead
    out[dead, 0] = 0.0
    out[dead, 4:] = np.eye(3)[UPPER]
    mu = m1[live] / m0[live, None]
    sig = m2[live] / m0[live, None, None] - mu[:, :, None] * mu[:, None, :]
    out[live, 1:4] = mu
    out[live, 4:] = sig[:, UPPER[0], UPPER[1]]
    return out


def log_likelihood(points, nodes, pre, j0, jn):
    """logLikelihood (:20-33): sum_i log(max(sum_{j in [j0, jn), pi_j >= eps} pi_j pdf_j(x_i), eps))."""
    pic, inv, _ = pre
    js = np.arange(j0, jn)
    js = js[nodes[js, 0] >= EPS]
    q = 0.0
    if js.size == 0:
        return points.shape[0] * np.log(EPS)
    step = max(1, BLOCK // js.size)
    for a in range(0, points.shape[0], step):
        x = points[a:a + step]
        tmp = _weighted_pdf(x[:, None, :], nodes[js, 1:4][None], inv[js][None], pic[js][None]).sum(axis=1)
        q += float(np.sum(np.log(np.maximum(tmp, EPS))))
    return q


def build(points, tree_level, idx, lambda_s=0.001, lambda_d=1.0e-4, max_iter=1000, trace=False):
    """buildGmmTree (:98-123).  Returns (nodes, info) with per level: iterations, the q of every iteration, the minimum
    top-two gamma gap of every E-step.  With ``trace`` also, per level and E-step, the m0 of all nodes ("m0") and the
    assignment ``current`` ("cur")."""
    points = np.asarray(points, dtype=np.float64)
    nodes = init_nodes(points, tree_level, idx)
    parent = -np.ones(points.shape[0], dtype=np.int64)
    info = {"iters": [], "q": [], "gap": []}
    if trace:
        info["m0"], info["cur"] = [], []
    for l in range(tree_level):
        prev_q = 0.0
        qs, gaps = [], []
        if trace:
            info["m0"].append([])
            info["cur"].append([])
        while True:
            pre = precompute(nodes)
            (m0, m1, m2), cur, gap = build_estep(points, nodes, pre, parent)
            lb, le = level(l), level(l + 1)
            if trace:
                info["m0"][l].append(m0.copy())
                info["cur"][l].append(cur.copy())
            nodes[lb:le] = ml_estimator(m0[lb:le], m1[lb:le], m2[lb:le], points.shape[0], lambda_d)
            q = log_likelihood(points, nodes, precompute(nodes), lb, le)
            qs.append(q)
            gaps.append(gap)
            if abs(q - prev_q) < lambda_s or len(qs) >= max_iter:
                break
            prev_q = q
        parent = cur
        info["iters"].append(len(qs))
        info["q"].append(qs)
        info["gap"].append(gaps)
    return nodes, info


def reg_estep(points, nodes, tree_level, lambda_c, return_gap=False):
    """gmmTreeRegEstep (:175-214) on already transformed points: (m0, m1, m2) per node."""
    points = np.asarray(points, dtype=np.float64)
    pic, inv, cplx = precompute(nodes)
    n = nodes.shape[0]
    m0, m1, m2 = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3, 3))
    gap = np.inf
    step = max(1, BLOCK // N_NODE)
    for a in range(0, points.shape[0], step):
        x = points[a:a + step]
        k = x.shape[0]
        search = -np.ones(k, dtype=np.int64)
        gsel = np.zeros(k)
        active = np.ones(k, dtype=bool)
        for _ in range(tree_level):
            ai = np.nonzero(active)[0]
            if ai.size == 0:
                break
            j = (search[ai, None] + 1) * N_NODE + np.arange(N_NODE)[None, :]
            g = _normalise(_weighted_pdf(x[ai, None, :], nodes[j, 1:4], inv[j], pic[j]))
            gap = min(gap, _top2_gap(g))
            best = np.argmax(g, axis=1)
            search[ai] = j[np.arange(ai.size), best]
            gsel[ai] = g[np.arange(ai.size), best]
            with np.errstate(invalid="ignore"):
                stop = cplx[search[ai]] <= lambda_c
            active[ai[stop]] = False
        m0 += np.bincount(search, gsel, minlength=n)
        for c in range(3):
            m1[:, c] += np.bincount(search, gsel * x[:, c], minlength=n)
            for d in range(3):
                m2[:, c, d] += np.bincount(search, gsel * x[:, c] * x[:, d], minlength=n)
    return ((m0, m1, m2), gap) if return_gap else (m0, m1, m2)


class OracleGmmTreePlan(object):
    """Stand-in for ``probreg_amd.gmmtree.GmmTreePlan`` (same methods, same array layouts)."""

    def __init__(self, device=None):
        self.tree_level = 0
        self.nodes = None
        self.target = None
        self.calls = []

    def close(self):
        pass

    def build(self, points, tree_level, idx, lambda_s, lambda_d, max_iter):
        self.nodes, info = build(points, tree_level, idx, lambda_s, lambda_d, max_iter)
        self.tree_level = tree_level
        qs = np.array([q[-1] for q in info["q"]])
        dq = np.array([abs(q[-1] - (q[-2] if len(q) > 1 else 0.0)) for q in info["q"]])
        return np.array(info["iters"], dtype=np.int32), qs, dq

    def set_nodes(self, arr, tree_level):
        self.nodes = np.array(arr, dtype=np.float64)
        self.tree_level = tree_level

    def get_nodes(self):
        return self.nodes.copy()

    def set_target(self, target):
        self.target = np.array(target, dtype=np.float64)

    def reg_estep(self, rot, t, scale, lambda_c, with_m2=False):
        self.calls.append((np.array(rot), np.array(t), float(scale)))
        x = scale * np.dot(self.target, np.asarray(rot).T) + t
        m0, m1, m2 = reg_estep(x, self.nodes, self.tree_level, lambda_c)
        m01 = np.concatenate([m0[:, None], m1], axis=1)
        return m01, (m2[:, UPPER[0], UPPER[1]] if with_m2 else None)


def nodes_as_tuples(nodes):
    """(n, 10) records -> the reference's NodeParamArray as pybind returns it: list of (pi, mu (3,), Sigma (3, 3))."""
    return [(float(r[0]), r[1:4].copy(), r[4:][SYM].copy()) for r in nodes]


def tuples_as_nodes(tuples):
    out = np.empty((len(tuples), 10))
    for j, (pi, mu, sig) in enumerate(tuples):
        out[j, 0] = pi
        out[j, 1:4] = mu
        out[j, 4:] = np.asarray(sig)[UPPER]
    return out


def standin_module(seed=0, max_iter=100000, record=None):
    """A ``probreg._gmmtree`` for the unmodified reference driver: build_gmmtree / gmmtree_reg_estep
    (cc/gmmtree_py.cc) on this restatement, leaf indices from ``init_indices(n, L, seed)``."""
    m = types.ModuleType("probreg._gmmtree")

    def build_gmmtree(points, tree_level, lambda_s, lambda_d):
        idx = init_indices(np.asarray(points).shape[0], tree_level, seed)
        nodes, info = build(points, tree_level, idx, lambda_s, lambda_d, max_iter)
        assert max(info["iters"]) < max_iter, "the build did not converge within %d iterations" % max_iter
        if record is not None:
            record.append({"idx": idx, "nodes": nodes, "info": info})
        return nodes_as_tuples(nodes)

    def gmmtree_reg_estep(target, nodes, tree_level, lambda_c):
        m0, m1, m2 = reg_estep(target, tuples_as_nodes(nodes), tree_level, lambda_c)
        return [(float(m0[j]), m1[j].copy(), m2[j].copy()) for j in range(m0.shape[0])]

    m.build_gmmtree = build_gmmtree
    m.gmmtree_reg_estep = gmmtree_reg_estep
    return m
