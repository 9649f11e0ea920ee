"""Extended-precision NumPy restatement of the mixture fit's stages (TEST INFRASTRUCTURE).

Written from the formulas in the header comment of probreg_amd/csrc/gmmfit.hip and from scikit-learn's documented
definitions of k-means++ (greedy variant), Lloyd's algorithm and the spherical ``GaussianMixture``:
  ``seed``              greedy k-means++ from explicit uniforms (k_seed_sweep, k_seed_choose)
  ``lloyd``             Lloyd iterations with the stop tests of prg_gmmfit_lloyd (k_assign, k_moments<true>, k_lloyd_update)
  ``init_from_labels``  the M-step on one-hot labels, weights = nk / N (prg_gmmfit_init_from_labels)
  ``em_step``           one EM iteration (k_normaliser, k_moments<false>, k_mstep, k_records)
Every difference, square, sum, exponential and logarithm is taken in ``np.longdouble`` (64-bit significand where the
platform has one, never less than fp64); the results the product stores in fp64 (centres, parameters) are rounded to
fp64 where the product stores them, so an iteration starts from the same numbers on both sides.  Neither a GPU nor
scikit-learn is imported, and it is never imported by the product.

Decisions.  Seeds, labels and iteration counts are integers, and a comparison of integers with the product means
something only where the decision behind each of them is not a matter of rounding.  ``seed`` and ``lloyd`` therefore
return the margins of their decisions next to the results; the tests assert on the margins before they compare.
``exact=True`` is for clouds built so that ties are exact (integer lattices, bitwise duplicates): a tie whose squared
distances are exactly representable in fp64 term by term is the same tie in any arithmetic and any summation order,
is broken by the documented first-minimum rule and is left out of the margins; any other tie counts as margin 0.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
TEN_EPS = 10.0 * EPS
LOG_2PI = np.log(2.0 * LD(np.pi))


def decision_bound(n):
    """16 N eps: N eps bounds the relative error of an N-term fp64 sum of same-signed terms in any order."""
    return 16.0 * n * EPS


def _points(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("points must be (n, dim)")
    return x, x.astype(LD)


def _d2(xl, c):
    """|x_i - c|^2 for every point, differences formed directly."""
    d = xl - np.asarray(c, dtype=LD)[None, :]
    return (d * d).sum(axis=1)


def _representable(v):
    return bool(np.all(v.astype(np.float64).astype(LD) == v))


def _same_sum(a, b):
    """True where sum(a) == sum(b) in fp64 whatever the order: the same terms point by point (bitwise duplicates), or
    integer terms on both sides whose sums stay below 2^53 and are equal."""
    if np.array_equal(a, b):
        return True
    whole = bool(np.all(a == np.rint(a)) and np.all(b == np.rint(b)))
    return whole and a.sum(dtype=LD) == b.sum(dtype=LD) and a.sum(dtype=LD) < LD(2.0 ** 53)


# ---- seeding ------------------------------------------------------------------------------------------------------------------
def seed(x, k, uniforms, exact=False):
    """Greedy k-means++.  ``uniforms`` is (k, trials) in [0, 1); entry [0, 0] draws the first centre.

    Returns ``(indices (k,) int64, margins)`` with margins ``{"winner": (k - 1,), "sampling": (k - 1,)}``:
      winner    (runner-up potential over distinct candidate indices - best) / best; inf with one distinct candidate
      sampling  min over the trials of |target - nearest inclusive cumulative sum| / total; inf where the total is 0
                (every point is a centre already: target 0, the first point is taken)
    With ``exact=True`` a candidate whose potential is the best one's in any arithmetic (``_same_sum``) is left out of
    the runner-up.
    """
    x, xl = _points(x)
    n = x.shape[0]
    u = np.asarray(uniforms, dtype=np.float64)
    trials = u.shape[1]
    idx = np.empty(k, dtype=np.int64)
    idx[0] = min(int(u[0, 0] * n), n - 1)
    mind2 = _d2(xl, xl[idx[0]])
    winner, sampling = np.full(k - 1, np.inf), np.full(k - 1, np.inf)
    for s in range(1, k):
        cum = np.cumsum(mind2, dtype=LD)
        total = cum[-1]
        targets = u[s].astype(LD) * total
        cand = np.minimum(np.searchsorted(cum, targets, side="left"), n - 1)  # first i with cum_i >= target
        if total > 0:
            sampling[s - 1] = float(min(np.min(np.abs(cum - t)) for t in targets) / total)
        new = [np.minimum(mind2, _d2(xl, xl[c])) for c in cand]
        pot = np.array([v.sum(dtype=LD) for v in new], dtype=LD)
        best = int(np.argmin(pot))  # first minimum
        others = [pot[l] for l in range(trials)
                  if cand[l] != cand[best] and not (exact and _same_sum(new[l], new[best]))]
        if others:
            gap = min(others) - pot[best]
            winner[s - 1] = float(gap / pot[best]) if pot[best] > 0 else (np.inf if gap > 0 else 0.0)
        idx[s] = cand[best]
        mind2 = new[best]
    return idx, {"winner": winner, "sampling": sampling}


def seed_brute_force(x, k, uniforms):
    """The same seeding by plain loops over points, with ``math.fsum`` and without a cumulative sum (for the oracle's own
    test): the candidate is the first point at which the exactly rounded sum of the leading squared distances reaches
    the target."""
    import math

    x = np.asarray(x, dtype=np.float64)
    n, dim = x.shape
    u = np.asarray(uniforms, dtype=np.float64)

    def d2(i, j):
        return math.fsum((x[i, d] - x[j, d]) ** 2 for d in range(dim))

    idx = [min(int(u[0, 0] * n), n - 1)]
    mind2 = [d2(i, idx[0]) for i in range(n)]
    for s in range(1, k):
        total = math.fsum(mind2)
        best, best_pot = -1, None
        for l in range(u.shape[1]):
            target = u[s, l] * total
            c = n - 1
            for i in range(n):
                if math.fsum(mind2[:i + 1]) >= target:
                    c = i
                    break
            pot = math.fsum(min(mind2[i], d2(i, c)) for i in range(n))
            if best_pot is None or pot < best_pot:
                best, best_pot = c, pot
        idx.append(best)
        mind2 = [min(mind2[i], d2(i, best)) for i in range(n)]
    return np.array(idx, dtype=np.int64)


# ---- Lloyd ---------------------------------------------------------------------------------------------------------------------
def _assign(xl, centers, xmax, exact):
    """Labels (first minimum) and the margins of the decisions: (labels, raw gap, gap / max(1, xmax / d))."""
    n, k = xl.shape[0], centers.shape[0]
    cl = centers.astype(LD)
    d2 = np.stack([_d2(xl, cl[j]) for j in range(k)], axis=1)
    labels = np.argmin(d2, axis=1)  # first minimum
    if k == 1:
        return labels, np.inf, np.inf
    two = np.partition(d2, 1, axis=1)[:, :2]
    d1, d2nd = two[:, 0], two[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(d2nd > 0, (d2nd - d1) / d2nd, LD(0))
    # d: the nearest distance; a point that is its centre bit for bit (a seed, a cluster of one) is at distance 0
    # in any arithmetic, and the distance that rounding can move is then the second one
    d = np.sqrt(np.where(d1 > 0, d1, d2nd))
    with np.errstate(divide="ignore"):
        clear = gap / np.maximum(LD(1), LD(xmax) / d)
    if exact:
        for i in np.nonzero(d2nd == d1)[0]:
            tied = np.nonzero(d2[i] == d1[i])[0]
            terms = (xl[i][None, :] - cl[tied]) ** 2
            sums = np.concatenate([terms.ravel(), np.cumsum(terms, axis=1).ravel(),
                                   np.cumsum(terms[:, ::-1], axis=1).ravel()])
            if _representable(sums):  # the same tie in fp64, whatever the order or the contraction of the sum
                gap[i] = clear[i] = np.inf
    return labels, float(np.min(gap)), float(np.min(clear))


def _label_sums(xl, labels, k):
    cnt = np.bincount(labels, minlength=k)
    order = np.argsort(labels, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(cnt)])
    return cnt, order, bounds


def lloyd(x, centers, max_iter, tol, exact=False):
    """Lloyd iterations from ``centers`` (k, dim).  label = nearest centre (first minimum); an empty cluster keeps its
    centre; stop when no label changed, else when the summed squared centre shift <= tol (the order of
    prg_gmmfit_lloyd); the labels are those of the final centres.

    Returns ``(centers, n_iter, counts, margins)``; ``margins`` holds
      label_gap    min over points and assignments of (d2_second - d2_nearest) / d2_second
      label_clear  min of that gap divided by max(1, max|x| / d), d the nearest distance of the decision: centres are
                   means of up to N coordinates of size max|x|, so d carries a relative error of N eps max|x| / d
      stop         min over iterations of |shift - tol| / tol (inf for a shift > 0 = tol, 0 for shift = tol)
      labels       the final labels (n,)
    """
    x, xl = _points(x)
    n, dim = x.shape
    c = np.array(centers, dtype=np.float64)
    k = c.shape[0]
    xmax = float(np.max(np.abs(x)))
    labels = -np.ones(n, dtype=np.int64)
    gap, clear, stop = np.inf, np.inf, np.inf
    strict, it = False, 0
    while it < max_iter:
        it += 1
        new, g, cl = _assign(xl, c, xmax, exact)
        gap, clear = min(gap, g), min(clear, cl)
        changed = int(np.count_nonzero(new != labels))
        labels = new
        cnt, order, bounds = _label_sums(xl, labels, k)
        shift = LD(0)
        for j in range(k):
            if cnt[j] > 0:
                mean = xl[order[bounds[j]:bounds[j + 1]]].sum(axis=0, dtype=LD) / LD(cnt[j])
                e = mean - c[j].astype(LD)
                shift += (e * e).sum()
                c[j] = mean.astype(np.float64)
        if changed == 0:
            strict = True
            break
        if tol > 0:
            margin = float(abs(shift - LD(tol)) / LD(tol))
        else:
            margin = np.inf if shift > 0 else 0.0
        if not (exact and margin == 0.0):
            stop = min(stop, margin)
        if shift <= tol:
            break
    if not strict:
        labels, g, cl = _assign(xl, c, xmax, exact)
        gap, clear = min(gap, g), min(clear, cl)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    return c, it, counts, {"label_gap": gap, "label_clear": clear, "stop": stop, "labels": labels}


# ---- M-step on labels, EM -------------------------------------------------------------------------------------------------------
def _mstep(s0, s1, s2, reg_covar):
    nk = s0 + LD(TEN_EPS)
    means = s1 / nk[:, None]
    cov = (s2 / nk[:, None] - means * means + LD(reg_covar)).mean(axis=1)
    return nk, means, cov


def init_from_labels(x, labels, k, reg_covar):
    """scikit-learn's start from one-hot responsibilities: nk = count + 10 eps, means = sum x / nk,
    cov = mean_d(sum x_d^2 / nk - means_d^2 + reg_covar), weights = nk / N.  Returns fp64 (weights, means, covariances)."""
    x, xl = _points(x)
    n, dim = x.shape
    labels = np.asarray(labels, dtype=np.int64)
    cnt, order, bounds = _label_sums(xl, labels, k)
    s1, s2 = np.zeros((k, dim), dtype=LD), np.zeros((k, dim), dtype=LD)
    for j in range(k):
        p = xl[order[bounds[j]:bounds[j + 1]]]
        s1[j] = p.sum(axis=0, dtype=LD)
        s2[j] = (p * p).sum(axis=0, dtype=LD)
    nk, means, cov = _mstep(cnt.astype(LD), s1, s2, reg_covar)
    return (nk / LD(n)).astype(np.float64), means.astype(np.float64), cov.astype(np.float64)


def em_step(x, weights, means, covariances, reg_covar, precisions=None):
    """One EM iteration from (weights, means, covariances), or from ``precisions`` = 1 / covariance where given
    (``covariances`` is then ignored; c = sqrt(precision) instead of 1 / sqrt(covariance)):
      log p(i, k) = log w_k + dim log c_k - dim / 2 log 2 pi - c_k^2 |x_i - mu_k|^2 / 2,
      normaliser_i = log sum_k exp(log p(i, k)) by log-sum-exp, resp = exp(log p - normaliser),
      nk = sum resp + 10 eps, means = sum resp x / nk, cov = mean_d(sum resp x_d^2 / nk - means_d^2 + reg_covar),
      weights = nk / sum nk, lower bound = mean normaliser (of the parameters the step starts from).
    Returns fp64 (weights, means, covariances, lower_bound)."""
    x, xl = _points(x)
    n, dim = x.shape
    w = np.asarray(weights, dtype=np.float64).astype(LD)
    mu = np.asarray(means, dtype=np.float64).astype(LD)
    k = w.shape[0]
    if precisions is not None:
        c = np.sqrt(np.asarray(precisions, dtype=np.float64).astype(LD))
    else:
        c = LD(1) / np.sqrt(np.asarray(covariances, dtype=np.float64).astype(LD))
    with np.errstate(divide="ignore"):
        const = np.log(w) + LD(dim) * np.log(c) - LD(0.5) * LD(dim) * LOG_2PI
    s0, s1, s2 = np.zeros(k, dtype=LD), np.zeros((k, dim), dtype=LD), np.zeros((k, dim), dtype=LD)
    total = LD(0)
    step = max(1, (1 << 21) // k)
    for a in range(0, n, step):
        xb = xl[a:a + step]
        logp = np.stack([const[j] - LD(0.5) * (c[j] * c[j]) * _d2(xb, mu[j]) for j in range(k)], axis=1)
        m = logp.max(axis=1)
        with np.errstate(under="ignore"):
            lse = m + np.log(np.exp(logp - m[:, None]).sum(axis=1, dtype=LD))
            r = np.exp(logp - lse[:, None])
        total += lse.sum(dtype=LD)
        s0 += r.sum(axis=0, dtype=LD)
        for d in range(dim):
            s1[:, d] += (r * xb[:, d:d + 1]).sum(axis=0, dtype=LD)
            s2[:, d] += (r * (xb[:, d:d + 1] * xb[:, d:d + 1])).sum(axis=0, dtype=LD)
    nk, mean, cov = _mstep(s0, s1, s2, reg_covar)
    return ((nk / nk.sum(dtype=LD)).astype(np.float64), mean.astype(np.float64), cov.astype(np.float64),
            float(total / LD(n)))
