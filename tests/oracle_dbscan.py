"""NumPy restatement of DESIGN.md section 3.19: DBSCAN with a canonical numbering, written from that definition and not from
csrc/icp_cluster.hip.

A brute-force d2 matrix (d2 = (dx dx + dy dy) + dz dz, one IEEE operation per step, as tests/oracle_knn.py), a sequential
union-find over the core points in index order and the border rule by np.lexsort on (d2, index).  Clouds of a few thousand
points: the matrix is n x n doubles.
"""
import numpy as np

from oracle_knn import cached, d2_block  # noqa: F401  (cached: the tests' one cache)


def pad3(points):
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float64))
    if p.shape[1] == 2:
        p = np.ascontiguousarray(np.concatenate([p, np.zeros((p.shape[0], 1))], axis=1))
    return p


def _find(parent, x):
    r = x
    while parent[r] != r:
        r = parent[r]
    while parent[x] != r:  # compress: the next find is short
        parent[x], x = r, parent[x]
    return r


def dbscan(points, eps, min_points):
    """dict: labels (n,) int32, core (n,) bool, counts (n,) int32, n_clusters, sizes (n_clusters,) int32, and
    ambiguous: the border points with core neighbours in more than one cluster; gap: the least |d2 - eps eps| / (eps eps)."""
    p = pad3(points)
    n = p.shape[0]
    e2 = eps * eps
    d2 = d2_block(p, p)
    near = d2 <= e2
    counts = np.sum(near, axis=1).astype(np.int32)
    core = counts >= min_points
    # the components of the core graph: a sequential union-find, the larger root under the smaller
    parent = np.arange(n)
    for i in np.nonzero(core)[0]:
        for j in np.nonzero(near[i, :i] & core[:i])[0]:
            a, b = _find(parent, i), _find(parent, j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    root = np.full(n, -1)
    for i in np.nonzero(core)[0]:
        root[i] = _find(parent, i)
    heads = np.nonzero(core & (root == np.arange(n)))[0]  # ascending: the smallest core index of every cluster
    ident = np.full(n, -1)
    ident[heads] = np.arange(heads.shape[0])
    labels = np.full(n, -1, dtype=np.int32)
    labels[core] = ident[root[core]]
    ambiguous = []
    ids = np.arange(n)
    for i in np.nonzero(~core)[0]:
        cand = np.nonzero(near[i] & core)[0]
        if cand.shape[0] == 0:
            continue
        order = np.lexsort((ids[cand], d2[i, cand]))  # by d2, then by index
        labels[i] = labels[cand[order[0]]]
        if np.unique(labels[cand]).shape[0] > 1:
            ambiguous.append(int(i))
    sizes = np.bincount(labels[labels >= 0], minlength=heads.shape[0]).astype(np.int32)
    return {"labels": labels, "core": core, "counts": counts, "n_clusters": int(heads.shape[0]), "sizes": sizes,
            "ambiguous": np.asarray(ambiguous, dtype=np.int64), "gap": float(np.min(np.abs(d2 - e2) / e2))}


def clusters(ref, min_size=1):
    """The ascending index arrays of the clusters with at least min_size members, in label order."""
    return [np.nonzero(ref["labels"] == c)[0].astype(np.int32) for c in range(ref["n_clusters"]) if ref["sizes"][c] >= min_size]
