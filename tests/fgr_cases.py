"""The shared inputs of the fast-global-registration tests (tests/oracle_fgr.py is the yardstick): synthetic and seeded.

A case is a 1500-point sample of the synthetic surface, the same points turned by rot_zx(140, 65), shifted and with noise
0.002 as the target, and C correspondences of which a stated share is wrong (a random partner).  The restatement's results
are computed once per case and shared; nothing here is ever written to.
"""
import functools

import numpy as np

import oracle_fgr as of
from oracle_global_reg import SHIFT

N_POINTS, NOISE, ROT_DEG = 1500, 0.002, (140.0, 65.0)
# name -> (C, share of wrong correspondences, seed): the loop cases of the GPU tests and the quality cases of the CPU tests
LOOP = {"wrong50": (600, 0.5, 0), "wrong70": (800, 0.7, 1), "wrong80": (1000, 0.8, 2)}
QUALITY = [(c, w, s) for c, w in ((600, 0.5), (800, 0.7), (1000, 0.8)) for s in (0, 1, 2)]
QUALITY_DEG, QUALITY_SHIFT = 0.5, 5.0e-3


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def clouds(seed):
    """(source, target, rot, t): the target is the moved source, row for row, plus noise."""
    from probreg_amd import synthetic

    rot = synthetic.rot_zx(*ROT_DEG)
    src = np.ascontiguousarray(synthetic.surface(N_POINTS, 40 + seed))
    tgt = src @ rot.T + SHIFT + np.random.default_rng(50 + seed).normal(0.0, NOISE, src.shape)
    return _frozen(src, np.ascontiguousarray(tgt), rot, SHIFT.copy())


@functools.lru_cache(maxsize=None)
def case(c, wrong, seed):
    """(source, target, corr (c, 2) int32, rot, t): c distinct source rows, round(wrong c) of them with a random other row
    of the target as the partner, the wrong ones scattered among the right ones."""
    src, tgt, rot, t = clouds(seed)
    rng = np.random.default_rng(60 + seed)
    i = rng.permutation(N_POINTS)[:c]
    j = i.copy()
    bad = rng.permutation(c)[:int(round(wrong * c))]
    j[bad] = (i[bad] + rng.integers(1, N_POINTS, bad.shape[0])) % N_POINTS
    corr = np.stack([i, j], axis=1).astype(np.int32)
    return (src, tgt) + _frozen(corr) + (rot, t)


@functools.lru_cache(maxsize=None)
def reference(c, wrong, seed, tuple_test=True):
    src, tgt, corr, _, _ = case(c, wrong, seed)
    return of.fgr(src, tgt, corr, tuple_test=tuple_test, seed=seed)


def exact_case(c=40, seed=3):
    """Exact correspondences without noise and without wrong ones: (source, target, corr, rot, t)."""
    rng = np.random.default_rng(70 + seed)
    src = rng.uniform(-1.0, 1.0, (c, 3))
    from oracle_global_reg import rotation_about
    rot = rotation_about((1.0, -2.0, 0.5), 0.4)
    t = np.array([0.3, -0.2, 0.1])
    return src, src @ rot.T + t, np.stack([np.arange(c), np.arange(c)], axis=1).astype(np.int32), rot, t


def pair_cloud(k, seed=0):
    """k pairs (p, q) of normalised size, a pose near them and a mu: the input of the sums tests."""
    from oracle_global_reg import rotation_about
    rng = np.random.default_rng(80 + seed + k)
    p = rng.uniform(-0.6, 0.6, (k, 3))
    rot = rotation_about((0.2, 1.0, -0.4), 0.3)
    q = p @ rot.T + np.array([0.05, -0.02, 0.03]) + rng.normal(0.0, 0.01, (k, 3))
    wrong = rng.permutation(k)[:k // 3]
    q[wrong] = rng.uniform(-0.6, 0.6, (wrong.shape[0], 3))
    pose = np.concatenate([rotation_about((0.1, 0.9, -0.3), 0.25).reshape(9), [0.04, -0.01, 0.02]])
    return np.ascontiguousarray(p), np.ascontiguousarray(q), pose, 0.37


def normalise_cloud(n, shift=0.0, seed=0):
    rng = np.random.default_rng(90 + seed + n)
    return np.ascontiguousarray(rng.uniform(-1.0, 1.0, (n, 3)) * np.array([1.0, 0.7, 0.4]) + shift)
