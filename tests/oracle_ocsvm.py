"""NumPy restatement of the one-class nu-SVM solve (csrc/ocsvm.hip), the yardstick of tests/test_ocsvm_gpu.py.

The dual in libsvm's scaling: minimise 1/2 a'Qa subject to 0 <= a_i <= 1 and sum a_i = nu n, Q_ij = exp(-gamma |x_i - x_j|^2).

  kernel / objective / kkt_gap / decision / rho   what a solution is judged by, from a dense fp64 Q
  smo                                              libsvm's Solver::Solve for this problem: WSS2 pair choice, clipping, the
                                                   stop test m - M < tol, from libsvm's start
  working_set_solve                                the decomposition of ocsvm.hip (group selection, SMO on the set, gradient
                                                   update), stage by stage, to count rounds and steps without a device

tests/test_oracle_ocsvm.py ties these to scikit-learn's recorded solutions (tests/golden/svr_golden.npz).
"""
import numpy as np

TAU = 1.0e-12


def kernel(x, y, gamma):
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for d in range(x.shape[1]):
        e = x[:, d, None] - y[None, :, d]
        d2 += e * e
    return np.exp(-gamma * d2)


def objective(x, gamma, alpha):
    sv = np.flatnonzero(alpha)
    return 0.5 * float(alpha[sv] @ kernel(x[sv], x[sv], gamma) @ alpha[sv])


def gradient(x, gamma, alpha):
    sv = np.flatnonzero(alpha)
    return kernel(x, x[sv], gamma) @ alpha[sv]


def gap_of(alpha, grad):
    """m - M with m = max over {a < 1} of -G and M = min over {a > 0} of -G; -inf when either set is empty."""
    up, low = alpha < 1.0, alpha > 0.0
    if not up.any() or not low.any():
        return -np.inf
    return float(np.max(-grad[up]) - np.min(-grad[low]))


def kkt_gap(x, gamma, alpha):
    return gap_of(alpha, gradient(x, gamma, alpha))


def decision(x, gamma, alpha, pts):
    """sum_i a_i k(x_i, p): scikit-learn's score_samples (decision_function is this minus rho)."""
    sv = np.flatnonzero(alpha)
    return kernel(pts, x[sv], gamma) @ alpha[sv]


def rho(x, gamma, alpha):
    """libsvm's calculate_rho: mean gradient over the free variables, else the midpoint of the two bounds."""
    grad = gradient(x, gamma, alpha)
    free = (alpha > 0.0) & (alpha < 1.0)
    if free.any():
        return float(np.mean(grad[free]))
    ub = np.min(grad[alpha <= 0.0]) if (alpha <= 0.0).any() else np.inf
    lb = np.max(grad[alpha >= 1.0]) if (alpha >= 1.0).any() else -np.inf
    return 0.5 * float(ub + lb)


def initial_alpha(n, nu):
    alpha = np.zeros(n)
    n_full = min(int(nu * n), n)
    alpha[:n_full] = 1.0
    if n_full < n:
        alpha[n_full] = nu * n - n_full
    return alpha


def _pair_step(ai, aj, gi, gj, kij):
    quad = 2.0 - 2.0 * kij
    if not quad > 0.0:
        quad = TAU
    delta = (gi - gj) / quad
    s = ai + aj
    ni, nj = ai - delta, aj + delta
    if s > 1.0:
        if ni > 1.0:
            ni, nj = 1.0, s - 1.0
    elif nj < 0.0:
        ni, nj = s, 0.0
    if s > 1.0:
        if nj > 1.0:
            ni, nj = s - 1.0, 1.0
    elif ni < 0.0:
        ni, nj = 0.0, s
    return ni, nj


def _smo_loop(q, alpha, grad, eps, max_steps):
    """WSS2 steps on (alpha, grad) in place until the gap < eps; (steps, gap at entry, gap at exit)."""
    gap0 = None
    it = 0
    while True:
        up, low = alpha < 1.0, alpha > 0.0
        gap = -np.inf
        if up.any() and low.any():
            i = int(np.argmax(np.where(up, -grad, -np.inf)))
            m = -grad[i]
            gap = m + np.max(grad[low])
        if gap0 is None:
            gap0 = gap
            if callable(eps):
                eps = eps(gap0)
        if not gap >= eps or it >= max_steps:
            return it, gap0, gap
        b = m + grad
        cand = low & (b > 0.0)
        quad = 2.0 - 2.0 * q[i]
        score = np.where(cand, b * b / np.where(quad > 0.0, quad, TAU), -np.inf)
        j = int(np.argmax(score))
        ni, nj = _pair_step(alpha[i], alpha[j], grad[i], grad[j], q[i, j])
        grad += (ni - alpha[i]) * q[i] + (nj - alpha[j]) * q[j]
        alpha[i], alpha[j] = ni, nj
        it += 1


def smo(x, gamma, nu, tol=1.0e-3, max_iter=10 ** 7):
    """libsvm's solve on the dense Q: (alpha, steps, converged)."""
    x = np.asarray(x, dtype=np.float64)
    q = kernel(x, x, gamma)
    alpha = initial_alpha(x.shape[0], nu)
    grad = q @ alpha
    it, _, gap = _smo_loop(q, alpha, grad, tol, max_iter)
    return alpha, it, bool(gap < tol)


def select_working_set(alpha, grad, q_size):
    """ocsvm.hip k_select: group g = {g, g + q/2, ...} gives its 'up' point with the largest -G (first of equals) and its
    'low' point with the smallest -G other than that one; -1 where there is none."""
    groups = q_size // 2
    ws = np.full(q_size, -1, dtype=np.int64)
    for g in range(groups):
        idx = np.arange(g, alpha.shape[0], groups)
        if idx.size == 0:
            continue
        up = alpha[idx] < 1.0
        ui = -1
        if up.any():
            ui = int(idx[np.argmax(np.where(up, -grad[idx], -np.inf))])
            ws[g] = ui
        low = (alpha[idx] > 0.0) & (idx != ui)
        if low.any():
            ws[groups + g] = int(idx[np.argmax(np.where(low, grad[idx], -np.inf))])
    return ws


def working_set_solve(x, gamma, nu, tol=1.0e-3, max_iter=100000, q_size=256, inner_cap=1024):
    """The rounds of ocsvm.hip: (alpha, rounds, steps, converged, gap)."""
    x = np.asarray(x, dtype=np.float64)
    alpha = initial_alpha(x.shape[0], nu)
    grad = gradient(x, gamma, alpha)
    rounds = steps = 0
    while True:
        gap = gap_of(alpha, grad)
        if not gap >= tol:
            return alpha, rounds, steps, True, gap
        if rounds >= max_iter:
            return alpha, rounds, steps, False, gap
        ws = select_working_set(alpha, grad, q_size)
        ws = ws[ws >= 0]
        qw = kernel(x[ws], x[ws], gamma)
        a, g = alpha[ws].copy(), grad[ws].copy()
        it, _, _ = _smo_loop(qw, a, g, lambda gap0: max(0.5 * tol, 0.1 * gap0), inner_cap)
        grad += kernel(x, x[ws], gamma) @ (a - alpha[ws])
        alpha[ws] = a
        rounds += 1
        steps += it
