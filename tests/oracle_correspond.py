"""numpy fp64 restatement of the CPD correspondences (TEST INFRASTRUCTURE): the dense posterior P of the reference's
E-step (probreg/cpd.py:71-88; weighted: probreg/bcpd.py:53-72) and its log-domain score, in chunks of owned points, and the k best
streamed points per owned point by a stable sort on (-score, index).

    a_m   = exp(log_weight_m)            (1 without weights)
    den_n = sum_m a_m exp(-|x_n - z_m|^2 / 2 sigma2);   den_n == 0 -> float32 eps (cpd.py:81);   then den_n += c (cpd.py:82)
    c     = (2 pi sigma2)^(D/2) w / (1 - w) ratio,   ratio = M / N or the caller's uniform_ratio
    P_mn  = a_m exp(-|x_n - z_m|^2 / 2 sigma2) / den_n
    s_mn  = log2 P_mn = b_n - kappa (|x_n - z_m|^2 + q_m),   kappa = log2(e) / 2 sigma2,  b_n = -log2 den_n,  q_m = -2 sigma2 ln a_m

Plain module: no pytest hooks, no fixtures, nothing here needs a GPU."""
from collections import namedtuple

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
LOG2E = 1.4426950408889634

Terms = namedtuple("Terms", ["z", "x", "sigma2", "kappa", "a", "q", "den", "b", "c", "zero"])
TopK = namedtuple("TopK", ["index", "score"])   # (owned, kk) each: the kk best streamed points, descending, ties by index


def _d2(p, r):
    d = p[:, None, :] - r[None, :, :]
    return np.einsum("mnd,mnd->mn", d, d)


def terms(z, x, sigma2, w=0.0, log_weights=None, uniform_ratio=0.0, chunk=512):
    """The per-point terms of the definition for the transformed source z (M, D) and the target x (N, D)."""
    z = np.asarray(z, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    m, dim = z.shape
    n = x.shape[0]
    lw = np.zeros(m) if log_weights is None else np.asarray(log_weights, dtype=np.float64)
    a = np.exp(lw)
    den = np.zeros(n)
    for s in range(0, m, chunk):
        den += (a[s:s + chunk, None] * np.exp(-_d2(z[s:s + chunk], x) / (2.0 * sigma2))).sum(axis=0)
    zero = den == 0
    den[zero] = EPS32
    ratio = uniform_ratio if uniform_ratio > 0.0 else m / n
    c = (2.0 * np.pi * sigma2) ** (dim * 0.5) * (w / (1.0 - w) * ratio) if w > 0.0 else 0.0
    den = den + c
    with np.errstate(divide="ignore"):
        q = -2.0 * sigma2 * lw
    return Terms(z, x, float(sigma2), LOG2E / (2.0 * sigma2), a, q, den, -np.log2(den), c, zero)


def posterior_rows(t, lo, hi):
    """P[lo:hi, :] (source rows) by the definition."""
    return t.a[lo:hi, None] * np.exp(-_d2(t.z[lo:hi], t.x) / (2.0 * t.sigma2)) / t.den[None, :]


def sums(t, chunk=512):
    """(pt1, p1) of the dense P."""
    pt1 = np.zeros(t.x.shape[0])
    p1 = np.empty(t.z.shape[0])
    for s in range(0, t.z.shape[0], chunk):
        p = posterior_rows(t, s, s + chunk)
        pt1 += p.sum(axis=0)
        p1[s:s + chunk] = p.sum(axis=1)
    return pt1, p1


def score_block(t, side, lo, hi):
    """s for the owned points lo:hi of `side` against every streamed point: (hi - lo, streamed)."""
    if side == "source":
        return t.b[None, :] - t.kappa * (_d2(t.z[lo:hi], t.x) + t.q[lo:hi, None])
    return t.b[lo:hi, None] - t.kappa * (_d2(t.x[lo:hi], t.z) + t.q[None, :])


def score_at(t, side, owned, streamed):
    """s of explicit (owned, streamed) index pairs (arrays of one shape)."""
    mi, ni = (owned, streamed) if side == "source" else (streamed, owned)
    d = t.z[mi] - t.x[ni]
    return t.b[ni] - t.kappa * (np.sum(d * d, axis=-1) + t.q[mi])


def kappa_d2_at(t, side, owned, streamed):
    """kappa d^2 of explicit pairs: the magnitude the relative term of the error budget acts on."""
    mi, ni = (owned, streamed) if side == "source" else (streamed, owned)
    d = t.z[mi] - t.x[ni]
    return t.kappa * np.sum(d * d, axis=-1)


def topk_of_scores(s, kk):
    """The kk best columns of every row of s by a stable sort on (-s, index) -> TopK; -inf / -1 fill rows shorter than kk."""
    rows, cols = s.shape
    take = min(kk, cols)
    if cols <= 4 * kk + 8:
        order = np.argsort(-s, axis=1, kind="stable")[:, :take]
    else:
        # candidates: everything at least as large as the take-th largest value (ties with it included); rows with more
        # candidates than `take` (a tie across the cut) go through the full stable sort
        part = np.argpartition(-s, take - 1, axis=1)[:, :take]
        part.sort(axis=1)                                        # candidate columns by index ...
        vals = np.take_along_axis(s, part, axis=1)
        inner = np.argsort(-vals, axis=1, kind="stable")         # ... then stably by score: ties keep the smaller index first
        order = np.take_along_axis(part, inner, axis=1)
        cut = np.take_along_axis(s, order[:, -1:], axis=1)
        tied = np.flatnonzero((s >= cut).sum(axis=1) > take)
        if tied.size:
            order[tied] = np.argsort(-s[tied], axis=1, kind="stable")[:, :take]
    score = np.take_along_axis(s, order, axis=1)
    if take < kk:
        order = np.concatenate([order, np.full((rows, kk - take), -1, dtype=order.dtype)], axis=1)
        score = np.concatenate([score, np.full((rows, kk - take), -np.inf)], axis=1)
    return TopK(order.astype(np.int64), score)


def topk(t, side, kk, chunk=256):
    """The kk best streamed points of every owned point of `side`."""
    owned = t.z.shape[0] if side == "source" else t.x.shape[0]
    idx, sc = [], []
    for lo in range(0, owned, chunk):
        r = topk_of_scores(score_block(t, side, lo, min(lo + chunk, owned)), kk)
        idx.append(r.index)
        sc.append(r.score)
    return TopK(np.concatenate(idx), np.concatenate(sc))


def stage_scores(owned, streamed, kappa, owned_bias=None, streamed_bias=None):
    """The plan-free stage's score in fp64: owned_bias + streamed_bias - kappa |owned - streamed|^2, (n_o, n_s)."""
    o = np.asarray(owned, dtype=np.float64)
    s = np.asarray(streamed, dtype=np.float64)
    ob = np.zeros(o.shape[0]) if owned_bias is None else np.asarray(owned_bias, dtype=np.float64)
    sb = np.zeros(s.shape[0]) if streamed_bias is None else np.asarray(streamed_bias, dtype=np.float64)
    return ob[:, None] + sb[None, :] - kappa * _d2(o, s)
