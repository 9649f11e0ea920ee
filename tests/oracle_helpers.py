"""TEST INFRASTRUCTURE - restatements of the stand-alone helpers of csrc/misc.hip (probreg_amd.math_utils, gauss_transform,
cost_functions), written from the definitions of the operations and not from the kernels, with the error bounds and the case
tables that tests/test_helpers_gpu.py uses.  tests/test_oracle_helpers.py pins every function here to what the project already
trusts (oracle/gauss_numpy.py, oracle/cpd_numpy.py, oracle/bcpd_numpy.py and the reference's own fixtures) and checks on the host
every condition the GPU comparisons rely on.  Never imported by probreg_amd/.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, "the restatements need an extended-precision long double (x86-64)"

U24 = 2.0 ** -24  # unit round-off of float32
U53 = 2.0 ** -53  # ... of float64
FLUSH32 = 2.0 ** -126  # smallest normal float32: v_exp_f32 may return 0 below it


# ----------------------------------------------------------------------------------------------------------------------------
# Gauss transform
# ----------------------------------------------------------------------------------------------------------------------------
def gauss_terms(source, target, weights, h, block=256):
    """For every (weight row, target): want = sum_j w_j e_ij, A = sum_j |w_j| e_ij, B = sum_j |w_j| e_ij a_ij with
    a_ij = |t_i - s_j|^2 / h^2 and e_ij = exp(-a_ij), all in long double.  ``weights`` is (s,) or (rows, s); the three results
    are (t,) or (rows, t) long double arrays."""
    s = np.asarray(source, dtype=np.float64).astype(LD)
    t = np.asarray(target, dtype=np.float64).astype(LD)
    w = np.asarray(weights, dtype=np.float64).astype(LD)
    one_row = w.ndim == 1
    w = np.atleast_2d(w)
    h2 = LD(h) * LD(h)
    want, big_a, big_b = (np.empty((t.shape[0], w.shape[0]), dtype=LD) for _ in range(3))
    for i0 in range(0, t.shape[0], block):
        d = t[i0:i0 + block, None, :] - s[None, :, :]
        a = np.sum(d * d, axis=2) / h2  # [block][s]
        e = np.exp(-a)
        want[i0:i0 + block] = e @ w.T
        big_a[i0:i0 + block] = e @ np.abs(w).T
        big_b[i0:i0 + block] = (e * a) @ np.abs(w).T
    if one_row:
        return want[:, 0], big_a[:, 0], big_b[:, 0]
    return want.T, big_a.T, big_b.T


def gauss_bound_f32(big_a, big_b, sum_abs_w):
    """Per-entry bound of the fp32 formulation (differences fp64 -> float32, squared distance, exponent and exp2 in float32,
    sums in fp64).  Each difference is rounded once: the squared distance gains about 4 units of 2^-24, kk and the product one
    each, so a term's exponent is off by about 6 x 2^-24 x a; v_exp_f32 is good to 1 ulp = 2 units; terms below 2^-126 are
    flushed.  The constants 8 and 4 leave a factor of 1.3 to 2 over that count."""
    return U24 * (8 * big_b + 4 * big_a) + FLUSH32 * sum_abs_w


def gauss_bound_f64(big_a, big_b, s):
    """The same count in fp64, plus the worst case of a sequential fma chain over ``s`` terms."""
    return U53 * (8 * big_b + (8 + s) * big_a)


def gauss_emulate_f32(source, target, weights, h):
    """NumPy emulation of the fp32 formulation: float32 differences from an fp64 subtraction, float32 squared distance,
    float32 ``kk = -log2(e) / h^2`` and product, ``np.exp2`` on float32, fp64 sum.  (rows, t) or (t,)."""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    d = (t[:, None, :] - s[None, :, :]).astype(np.float32)
    d2 = d[:, :, 0] * d[:, :, 0]
    for k in range(1, d.shape[2]):
        d2 = d2 + d[:, :, k] * d[:, :, k]
    kk = np.float32(-1.4426950408889634 / (h * h))
    with np.errstate(under="ignore"):
        e = np.exp2(kk * d2).astype(np.float64)
    return (e @ np.atleast_2d(w).T).T if w.ndim == 2 else e @ w


def gauss_plain_f64(source, target, weights, h):
    """Plain fp64 evaluation of the definition.  (rows, t) or (t,)."""
    s = np.asarray(source, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    d = t[:, None, :] - s[None, :, :]
    e = np.exp(-np.sum(d * d, axis=2) / (h * h))
    return (e @ np.atleast_2d(w).T).T if w.ndim == 2 else e @ w


GAUSS_H = 0.35
GAUSS_SIZES = [(s, 70) for s in (1, 3, 4, 5, 255, 256, 257)] + [(70, t) for t in (1, 255, 256, 257, 513)]
GAUSS_ROWS = list(range(1, 10))
L2_SIZES = [1, 255, 256, 257]
L2_SIGMA = 0.25


def gauss_case(s, t, dim, rows=1, seed=0):
    """source (s, dim), target (t, dim), signed weights ((s,) for rows == 1, else (rows, s)) and h.  Even targets sit within
    about h of a source point, counted down from the LAST one (target 0 is beside source s - 1: a dropped tail shows there, and
    a < 1); odd targets are spread 1.5 times as wide as the source (a > 60 for many pairs)."""
    rng = np.random.default_rng([1000 + seed, s, t, dim, rows])
    source = rng.normal(size=(s, dim))
    target = 1.5 * rng.normal(size=(t, dim))
    near = np.arange(0, t, 2)
    target[near] = source[(s - 1 - near // 2) % s] + 0.4 * GAUSS_H * rng.normal(size=(near.size, dim))
    w = rng.uniform(0.25, 1.0, size=(rows, s)) * rng.choice([-1.0, 1.0], size=(rows, s))
    return source, target, (w[0] if rows == 1 else w), GAUSS_H


def l2_case(k, dim, seed=0):
    """mu_source, phi_source, mu_target, phi_target, sigma of a K x K ``compute_l2_dist`` (1 + dim weight rows)."""
    rng = np.random.default_rng([2000 + seed, k, dim])
    mu_t = rng.normal(size=(k, dim))
    mu_s = mu_t[::-1] + 0.3 * rng.normal(size=(k, dim))
    phi_s = rng.uniform(0.5, 1.5, k)
    phi_t = rng.uniform(0.5, 1.5, k)
    return mu_s, phi_s / phi_s.sum(), mu_t, phi_t / phi_t.sum(), L2_SIGMA


def l2_terms(mu_source, phi_source, mu_target, phi_target, sigma, bound):
    """``compute_l2_dist`` (cost_functions.py:33-41 of the reference) in long double from ``gauss_terms``, with the bound of the
    Gauss transform carried through its two lines of host algebra.  ``bound(A, B)`` is the per-entry bound of one transform.

    The transform has rows r_0 (weights phi_t / z) and r_k (weights phi_t mu_t[:, k] / z) evaluated at the source means, with
    errors |dr_0| <= b_0 and |dr_k| <= b_k per entry.  Then
        f = -sum_i phi_s_i r_0i                           |df|    <= sum_i phi_s_i b_0i
        g_ik = phi_s_i (r_0i mu_s_ik - r_ki) / (2 s^2)    |dg_ik| <= phi_s_i (b_0i |mu_s_ik| + b_ki) / (2 s^2)
    plus the fp64 rounding of the host algebra itself.  g: two products in the first term, one in the second, the difference and
    the division - at most 4 x 2^-53 phi_s_i (|r_0i mu_s_ik| + |r_ki|) / (2 s^2).  f: a product per term and a sum of K terms -
    at most (K + 2) x 2^-53 sum_i phi_s_i |r_0i|.
    Returns f, f_bound, g, g_bound."""
    mu_s = np.asarray(mu_source, dtype=np.float64)
    mu_t = np.asarray(mu_target, dtype=np.float64)
    k, dim = mu_s.shape
    # the weights the device receives are the caller's fp64 ones: formed in fp64 here too, the transform in long double
    z = np.power(2.0 * np.pi * sigma ** 2, dim * 0.5)
    weights = np.concatenate([(phi_target / z)[None, :], phi_target * mu_t.T / z], axis=0)
    r, big_a, big_b = gauss_terms(mu_t, mu_s, weights, np.sqrt(2.0) * sigma)
    b = bound(big_a, big_b)
    ps = np.asarray(phi_source, dtype=np.float64).astype(LD)
    ms = mu_s.astype(LD)
    two_s2 = LD(2.0 * sigma ** 2)
    f = -np.sum(ps * r[0])
    f_bound = np.sum(ps * b[0]) + (k + 2) * U53 * np.sum(ps * np.abs(r[0]))
    g = (ps[:, None] * (r[0][:, None] * ms - r[1:].T)) / two_s2
    g_bound = ps[:, None] * (b[0][:, None] * np.abs(ms) + b[1:].T) / two_s2
    g_bound = g_bound + 4 * U53 * ps[:, None] * (np.abs(r[0][:, None] * ms) + np.abs(r[1:].T)) / two_s2
    return f, f_bound, g, g_bound


# ----------------------------------------------------------------------------------------------------------------------------
# squared_kernel_sum
# ----------------------------------------------------------------------------------------------------------------------------
def sks_pairwise(x, y, block_elems=1 << 21):
    """(sum_mn |x_m - y_n|^2 / (M D N), U) from the differences themselves, in long double, in row blocks of the longer cloud.
    U = (n sum|x|^2 + m sum|y|^2 + 2 sum_k |sum x_k sum y_k|) / (M D N) is the magnitude of the closed form's terms before
    they cancel."""
    x = np.asarray(x, dtype=np.float64).astype(LD)
    y = np.asarray(y, dtype=np.float64).astype(LD)
    m, d = x.shape
    n = y.shape[0]
    long_, short = (x, y) if m >= n else (y, x)
    step = max(1, block_elems // (short.shape[0] * d))
    total = LD(0)
    for i0 in range(0, long_.shape[0], step):
        df = long_[i0:i0 + step, None, :] - short[None, :, :]
        total += np.sum(df * df)
    den = LD(m) * d * n
    u = (n * np.sum(x * x) + m * np.sum(y * y) + 2 * np.sum(np.abs(x.sum(axis=0) * y.sum(axis=0)))) / den
    return total / den, u


def sks_unshifted_f64(x, y):
    """The closed form n sum|x|^2 + m sum|y|^2 - 2 sum x . sum y in fp64 on float32-rounded, un-shifted coordinates: what
    ``squared_kernel_sum`` evaluated before it centred its clouds.  Kept to put that formulation's error on record."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    m, d = x.shape
    n = y.shape[0]
    return (n * np.sum(x * x) + m * np.sum(y * y) - 2.0 * np.dot(x.sum(axis=0), y.sum(axis=0))) / (m * d * n)


SKS_SHAPES = [(1, 1), (1, 257), (63, 64), (255, 256), (257, 255)]
SKS_DIMS = [1, 2, 3, 4, 33, 64]
SKS_STRIDED = [(65537, 300, 3), (131073, 300, 4)]  # one point more than 256 x 256 and 512 x 256: the lanes stride
SKS_FAR_SHAPES = [(700, 900), (5000, 3000)]
SKS_FAR_OFFSETS = {"z1277": (0.0, 0.0, 1277.0), "1e4": (1e4,) * 3, "1e5": (1e5,) * 3, "1e6": (1e6,) * 3}


def grid_cloud(n, dim, seed, bits=10, extent=4.0):
    """float32-exact cloud: multiples of 2^-bits in [-extent, extent), as float64.  Differences of two such clouds, and a
    cloud minus any of its points, are float32-exact too."""
    rng = np.random.default_rng([3000 + seed, n, dim])
    q = 2 ** bits
    return rng.integers(-int(extent * q), int(extent * q), size=(n, dim)).astype(np.float64) / q


def far_pair(m, n, dim, offset, seed=0):
    """fp64 clouds of unit extent moved by ``offset`` (the sum is rounded to fp64: these are the caller's inputs)."""
    rng = np.random.default_rng([4000 + seed, m, n, dim])
    x = rng.uniform(-0.5, 0.5, size=(m, dim))
    y = rng.uniform(-0.5, 0.5, size=(n, dim)) * np.linspace(0.6, 1.0, dim) + 0.1
    off = np.broadcast_to(np.asarray(offset, dtype=np.float64), (dim,))
    return x + off, y + off


# ----------------------------------------------------------------------------------------------------------------------------
# rbf_kernel, inverse_multiquadric_kernel
# ----------------------------------------------------------------------------------------------------------------------------
def _d2_f32(x, y):
    """float32 ((dx dx + dy dy) + dz dz), every operation rounded on its own (no fused multiply-add)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    d = x[:, None, :] - y[None, :, :]
    d2 = d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]
    if x.shape[1] > 2:
        d2 = d2 + d[:, :, 2] * d[:, :, 2]
    assert d2.dtype == np.float32
    return d2


def rbf_f32(x, y, beta):
    """(K, fragile): K_ij = exp(-d2 / (2 beta)) as the comment on k_rbf (csrc/misc.hip) documents it - d2 in float32 without
    fused multiply-add, ``arg = -d2 / float32(2 beta)`` in float32, the exponential in fp64 rounded once to float32.  ``fragile``
    marks the entries whose fp64 exponential lies within a relative 2^-46 of the midpoint of two adjacent float32 values: an
    fp64 ``exp`` that is 1-2 ulp off may round the other way there."""
    arg = (-_d2_f32(x, y)) / np.float32(2.0 * beta)
    assert arg.dtype == np.float32
    with np.errstate(under="ignore"):
        return round_f32_fragile(np.exp(arg.astype(np.float64)))


def round_f32_fragile(v):
    """(float32(v), fragile) for fp64 ``v``: fragile where v is within a relative 2^-46 of the midpoint between float32(v) and
    its float32 neighbour on v's side."""
    with np.errstate(under="ignore"):
        k = v.astype(np.float32)
    k64 = k.astype(np.float64)
    toward = np.where(v >= k64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    mid = 0.5 * (k64 + np.nextafter(k, toward).astype(np.float64))  # exact in fp64
    return k, (v != k64) & (np.abs(v - mid) <= 2.0 ** -46 * np.abs(v))


def imq_f32(x, y, c):
    """K_ij = 1 / sqrt(d2 + c) with every operation a correctly rounded float32 one (NumPy's float32 sqrt and / are)."""
    k = np.float32(1.0) / np.sqrt(_d2_f32(x, y) + np.float32(c))
    assert k.dtype == np.float32
    return k


KERNEL_M = [1, 15, 16, 17, 33]
KERNEL_N = [1, 255, 256, 257]
RBF_BETAS = [0.06, 2.0]
IMQ_CS = [0.7, 1.0]


def kernel_case(m, n, dim, seed=0):
    """float32 clouds (m, dim) and (n, dim)."""
    rng = np.random.default_rng([5000 + seed, m, n, dim])
    return rng.normal(size=(m, dim)).astype(np.float32), rng.normal(size=(n, dim)).astype(np.float32)


def kernel_square_case(dim, seed=0):
    return np.random.default_rng([5100 + seed, dim]).normal(size=(257, dim)).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------------------------
# compute_rmse
# ----------------------------------------------------------------------------------------------------------------------------
def nn_mean(source, target):
    """Mean nearest-neighbour distance as ``compute_rmse`` conditions it: both clouds minus the target's fp64 mean, rounded to
    float32; then the fp64 mean of the cKDTree distances between those rounded points."""
    from scipy.spatial import cKDTree

    tgt = np.asarray(target, dtype=np.float64)
    src = np.asarray(source, dtype=np.float64)
    c = tgt.mean(axis=0)
    a = (src - c).astype(np.float32).astype(np.float64)
    b = (tgt - c).astype(np.float32).astype(np.float64)
    return float(np.mean(cKDTree(b).query(a)[0]))


RMSE_TOL = 2.0 ** -21  # float32 squared distance of exact float32 points: ~5 x 2^-24; the root halves it; the mean is fp64
RMSE_SIZES = [(70, n) for n in (1, 3, 4, 5, 255, 256, 257, 513)] + [(m, 600) for m in (1, 255, 256, 257)]
RMSE_MANY_BLOCKS = (524289, 300)  # more than 2048 source blocks: one target segment


def rmse_case(m, n, dim, seed=0):
    rng = np.random.default_rng([6000 + seed, m, n, dim])
    return rng.normal(size=(m, dim)), rng.normal(size=(n, dim)) + 0.05


def nn_segments(m, n):
    """(nseg, seg_len): how ``prg_nn_mean_distance`` (csrc/misc.hip) cuts a target of n points for m sources.  The planted
    cases below sit on the edges of these segments."""
    nbx = -(-m // 256)
    nseg = min(max(1, 2048 // nbx), -(-n // 256))
    seg_len = -(-(-(-n // nseg)) // 4) * 4
    return nseg, seg_len


PLANT_M, PLANT_N = 64, 1025


def planted_case(dim, where):
    """64 sources whose nearest target is ONE planted point (the origin) at index ``where`` of 1025 targets, at the exactly
    representable distances 5 k / 8 (offsets (3 k, 4 k) / 8 with signs and axes varied, k = 1..8).  The other 1024 targets are
    +- pairs of grid points 16 to 32 away from the origin, so the target's mean is exactly 0 and ``compute_rmse``'s centring
    changes nothing.  Returns source, target, expected mean."""
    rng = np.random.default_rng([7000, dim])
    src, dist = [], []
    for k in range(1, 9):
        for v in range(8):
            a, b = (3.0 * k / 8, 4.0 * k / 8) if v & 1 else (4.0 * k / 8, 3.0 * k / 8)
            p = np.zeros(dim)
            i, j = (0, 1) if dim == 2 else [(0, 1), (1, 2), (0, 2), (2, 0)][v >> 1 & 3]
            p[i] = a if v & 2 else -a
            p[j] = b if v & 4 else -b
            src.append(p)
            dist.append(5.0 * k / 8)
    half = rng.integers(16 * 64, 32 * 64, size=(512, dim)).astype(np.float64) / 64
    half *= rng.choice([-1.0, 1.0], size=half.shape)
    back = np.concatenate([half, -half], axis=0)[rng.permutation(1024)]
    tgt = np.insert(back, where, np.zeros(dim), axis=0)
    return np.asarray(src), tgt, float(np.mean(dist))
