"""NumPy restatement of fast global registration as DESIGN.md section 3.21 defines it (normalisation, the tuple test, the
line-process sums, the Gauss-Newton step, the schedule of mu, the way back to the caller's units), written from that
definition and not from csrc/fgr.hip or csrc/fgr.h.

Every value the definition orders is one IEEE operation per step in that order; sums run over rows in ascending order inside
runs of RUN rows and the run sums are added in ascending order.  The entries of J^T J and J^T r are formed here from the full
3 x 6 Jacobian, zeros and ones included, which gives the bits of the definition's shortened forms (a product with 0 or 1 and
an addition of 0 are exact).  The draw is section 3.13's and is imported, not copied.
"""
import numpy as np

from oracle_global_reg import draw, solve_bound

RUN = 64                 # rows per run of every ordered sum
PIVOT = 1.0e-12          # a Cholesky pivot <= PIVOT max diag(A) is degenerate
TRIALS_PER_PAIR = 100    # the tuple test looks at trials t < 100 C
OK, TOO_FEW, DEGENERATE = "ok", "too_few", "degenerate"
IDENTITY = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def ordered_sum(rows):
    """Column sums of rows (n, k): ascending inside runs of RUN rows, then the runs in ascending order."""
    rows = np.asarray(rows, dtype=np.float64)
    n, k = rows.shape
    nruns = -(-n // RUN)
    pad = np.zeros((nruns * RUN, k))  # + 0.0 is exact and an accumulator that starts at + 0.0 never holds - 0.0
    pad[:n] = rows
    pad = pad.reshape(nruns, RUN, k)
    acc = np.zeros((nruns, k))
    for j in range(RUN):
        acc = acc + pad[:, j, :]
    total = np.zeros(k)
    for r in range(nruns):
        total = total + acc[r]
    return total


# ----------------------------------------------------------------------------------------------------------- normalise
def _dist2(x, mean):
    d = x - mean
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def normalise(source, target, use_absolute_scale=False):
    """(mean_p, mean_q, scale, scale_global, mu0)."""
    mean_p = ordered_sum(source) / float(source.shape[0])
    mean_q = ordered_sum(target) / float(target.shape[0])
    scale = float(np.sqrt(max(np.max(_dist2(source, mean_p)), np.max(_dist2(target, mean_q)))))
    return mean_p, mean_q, scale, (1.0 if use_absolute_scale else scale), (scale if use_absolute_scale else 1.0)


def pairs(source, target, corr, mean_p, mean_q, scale_global):
    """The matched points in normalised coordinates: (p (C, 3), q (C, 3))."""
    return (source[corr[:, 0]] - mean_p) / scale_global, (target[corr[:, 1]] - mean_q) / scale_global


# -------------------------------------------------------------------------------------------------------------- tuples
def _edge(x, a, b):
    d = x[a] - x[b]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def trial_passes(p, q, tri, s):
    ok = np.ones(tri.shape[0], dtype=bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        li, lj = _edge(p, tri[:, a], tri[:, b]), _edge(q, tri[:, a], tri[:, b])
        ok &= (li * s < lj) & (lj * s < li)
    return ok


def tuples(p, q, seed, tuple_scale=0.95, maximum_tuple_count=1000, block=50000):
    """(used (3 n_tuples,) int32, n_tuples, n_trials): the first ``maximum_tuple_count`` passing trials in ascending t."""
    c = p.shape[0]
    limit = TRIALS_PER_PAIR * c
    used, n_tuples, n_trials = [], 0, limit
    for t0 in range(0, limit, block):
        t = np.arange(t0, min(t0 + block, limit), dtype=np.uint64)
        tri = draw(seed, t, c)
        hit = np.nonzero(trial_passes(p, q, tri, tuple_scale))[0][:maximum_tuple_count - n_tuples]
        used.append(tri[hit].reshape(-1))
        n_tuples += hit.shape[0]
        if n_tuples == maximum_tuple_count:
            n_trials = t0 + int(hit[-1]) + 1
            break
    used = np.concatenate(used).astype(np.int32) if used else np.zeros(0, dtype=np.int32)
    return used, n_tuples, n_trials


# ------------------------------------------------------------------------------------------------------------ optimise
def moved(p, pose):
    """s_a = ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) + t_a."""
    s = np.empty_like(p)
    for a in range(3):
        s[:, a] = ((pose[3 * a] * p[:, 0] + pose[3 * a + 1] * p[:, 1]) + pose[3 * a + 2] * p[:, 2]) + pose[9 + a]
    return s


def weight(mu, r2):
    w = mu / (mu + r2)
    return w * w


def jacobian(s):
    """(K, 3, 6): row a of pair k is the derivative of r_a against the twist (omega, v): (-[s]x | I)."""
    k = s.shape[0]
    j = np.zeros((k, 3, 6))
    j[:, 0, 1], j[:, 0, 2] = s[:, 2], -s[:, 1]
    j[:, 1, 0], j[:, 1, 2] = -s[:, 2], s[:, 0]
    j[:, 2, 0], j[:, 2, 1] = s[:, 1], -s[:, 0]
    j[:, 0, 3] = j[:, 1, 4] = j[:, 2, 5] = 1.0
    return j


def pair_terms(p, q, pose, mu):
    """(terms (K, 28), l (K,)): what every pair adds to A's upper triangle (row-major, 21), to g (6) and to the objective."""
    s = moved(p, pose)
    r = s - q
    r2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    l = weight(mu, r2)
    j = jacobian(s)
    out = np.empty((p.shape[0], 28))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            out[:, k] = l * ((j[:, 0, a] * j[:, 0, b] + j[:, 1, a] * j[:, 1, b]) + j[:, 2, a] * j[:, 2, b])
            k += 1
    for a in range(6):
        out[:, 21 + a] = l * ((j[:, 0, a] * r[:, 0] + j[:, 1, a] * r[:, 1]) + j[:, 2, a] * r[:, 2])
    root = 1.0 - np.sqrt(l)
    out[:, 27] = l * r2 + mu * (root * root)
    return out, l


def sums(p, q, pose, mu):
    """The 28 raw sums over the pairs (p, q) (the used ones) at ``pose`` and ``mu``."""
    if p.shape[0] == 0:
        return np.zeros(28)
    return ordered_sum(pair_terms(p, q, pose, mu)[0])


def weights(p, q, pose, mu):
    return pair_terms(p, q, pose, mu)[1] if p.shape[0] else np.zeros(0)


def _unpack(s):
    a = np.zeros((6, 6))
    k = 0
    for i in range(6):
        for j in range(i, 6):
            a[i, j] = a[j, i] = s[k]
            k += 1
    return a, -s[21:27]


def cholesky(a, b):
    """x of a x = b by Cholesky, every inner product accumulated in ascending order; None when a pivot is <= PIVOT max diag."""
    low = np.zeros((6, 6))
    floor = PIVOT * max(0.0, np.max(np.diag(a)))
    for k in range(6):
        d = a[k, k]
        for j in range(k):
            d -= low[k, j] * low[k, j]
        if not d > floor:
            return None
        low[k, k] = np.sqrt(d)
        for i in range(k + 1, 6):
            v = a[i, k]
            for j in range(k):
                v -= low[i, j] * low[k, j]
            low[i, k] = v / low[k, k]
    w = np.zeros(6)
    for i in range(6):
        v = b[i]
        for j in range(i):
            v -= low[i, j] * w[j]
        w[i] = v / low[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        v = w[i]
        for j in range(i + 1, 6):
            v -= low[j, i] * x[j]
        x[i] = v / low[i, i]
    return x


def delta_from_x(x):
    """Open3D's TransformVector6dToMatrix4d: Rz(x2) Ry(x1) Rx(x0) row-major, then the shift x[3:]."""
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    return np.array([cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                     sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                     -sb, cb * sa, cb * ca, x[3], x[4], x[5]])


def compose(d, pose):
    """d pose: R <- dR R, t <- dR t + dt, each entry (a b + c d) + e f [+ g]."""
    out = np.empty(12)
    for a in range(3):
        for b in range(3):
            out[3 * a + b] = (d[3 * a] * pose[b] + d[3 * a + 1] * pose[3 + b]) + d[3 * a + 2] * pose[6 + b]
        out[9 + a] = ((d[3 * a] * pose[9] + d[3 * a + 1] * pose[10]) + d[3 * a + 2] * pose[11]) + d[9 + a]
    return out


def step(pose, s, n_used):
    """(new pose or None, status, disagreement): the step from the raw sums ``s`` of ``n_used`` pairs and the largest
    difference of the 12 pose entries from a second, independent host solve (least squares) of the same sums."""
    if n_used < 3:
        return None, TOO_FEW, 0.0
    a, b = _unpack(s)
    x = cholesky(a, b)
    if x is None:
        return None, DEGENERATE, 0.0
    new = compose(delta_from_x(x), pose)
    other = compose(delta_from_x(np.linalg.lstsq(a, b, rcond=None)[0]), pose)
    return new, OK, float(np.max(np.abs(new - other)))


def next_mu(mu, i, decrease_mu=True, division_factor=1.4, maximum_correspondence_distance=0.025):
    """mu after iteration i (counted from 0)."""
    if decrease_mu and i % 4 == 0 and mu > maximum_correspondence_distance:
        return mu / division_factor
    return mu


def _one_ulp(pose, rng):
    up = rng.integers(0, 2, 12).astype(bool)
    return np.where(up, np.nextafter(pose, np.inf), np.nextafter(pose, -np.inf))


def optimise(p, q, iteration_number=64, division_factor=1.4, decrease_mu=True, maximum_correspondence_distance=0.025,
             mu=1.0, pose=None, perturb=None):
    """The loop on the used pairs (p, q): dict of pose, mu, the sequence of mu (one entry per step done), n_iter, status, the
    objective of the last sums, the final weights and the largest disagreement of the two host solves of a step.
    ``perturb``: a NumPy generator; every pose entry is then moved by one ulp up or down after each step (the experiment the
    GPU loop's tolerance comes from)."""
    pose = IDENTITY.copy() if pose is None else np.array(pose, dtype=np.float64).reshape(12)
    mus, status, worst, objective, n_iter = [], OK, 0.0, 0.0, 0
    for i in range(iteration_number):
        s = sums(p, q, pose, mu)
        objective = float(s[27])
        new, status, dis = step(pose, s, p.shape[0])
        if new is None:
            break
        pose = new if perturb is None else _one_ulp(new, perturb)
        worst = max(worst, dis)
        mu = next_mu(mu, i, decrease_mu, division_factor, maximum_correspondence_distance)
        mus.append(mu)
        n_iter += 1
    if p.shape[0] < 3:
        status = TOO_FEW
    return {"pose": pose, "mu": mu, "mus": np.array(mus), "n_iter": n_iter, "status": status, "objective": objective,
            "weights": weights(p, q, pose, mu), "disagreement": worst}


# ---------------------------------------------------------------------------------------------------------- whole call
def denormalise(pose, mean_p, mean_q, scale_global):
    """R stays; t_out_a = (scale_global t_a + mean_q_a) - ((R_a0 m_0 + R_a1 m_1) + R_a2 m_2) with m = mean_p."""
    out = pose.copy()
    for a in range(3):
        rm = (pose[3 * a] * mean_p[0] + pose[3 * a + 1] * mean_p[1]) + pose[3 * a + 2] * mean_p[2]
        out[9 + a] = (scale_global * pose[9 + a] + mean_q[a]) - rm
    return out


def fgr(source, target, corr, maximum_correspondence_distance=0.025, iteration_number=64, division_factor=1.4,
        decrease_mu=True, use_absolute_scale=False, tuple_test=True, tuple_scale=0.95, maximum_tuple_count=1000, seed=0,
        perturb=None):
    """The whole definition: the dict of ``optimise`` plus used, n_tuples, n_trials, the normalisation, the used pairs
    (up, uq) and pose_out / rot / t in the caller's units."""
    corr = np.asarray(corr)
    mean_p, mean_q, scale, sg, mu0 = normalise(source, target, use_absolute_scale)
    p, q = pairs(source, target, corr, mean_p, mean_q, sg)
    if tuple_test:
        used, n_tuples, n_trials = tuples(p, q, seed, tuple_scale, maximum_tuple_count)
    else:
        used, n_tuples, n_trials = np.arange(corr.shape[0], dtype=np.int32), 0, 0
    up, uq = p[used], q[used]
    out = optimise(up, uq, iteration_number, division_factor, decrease_mu, maximum_correspondence_distance, mu0, perturb=perturb)
    pose_out = denormalise(out["pose"], mean_p, mean_q, sg)
    out.update(used=used, n_tuples=n_tuples, n_trials=n_trials, mean_p=mean_p, mean_q=mean_q, scale=scale, scale_global=sg,
               up=up, uq=uq, pose_out=pose_out, rot=pose_out[:9].reshape(3, 3), t=pose_out[9:])
    return out


def step_bound(disagreement):
    """What a third fp64 solve of a step may differ by (the bound of the ICP step tests)."""
    return solve_bound(disagreement)
