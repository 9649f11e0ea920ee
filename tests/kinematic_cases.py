"""Clouds of the deformable kinematic tests: the "clustered bar" and the reference's example.

The bar: 60 centres uniform in [0,1] x [0,0.3] x [0,0.2], every point a random centre plus 0.015 N(0, I); K nodes evenly
spaced along x, every point tied to the two nodes around it with linear weights (1 - u, u) stored as float32, every other
point with its pair order reversed.  Node k rotates by 2 deg (k + 1) about (0, 0.2, 1) and moves by (k + 1) (0.005, 0,
0.0075), times ``motion``.  (A uniform flat sheet slides within its plane and registers poorly: not used.)
"""
from collections import namedtuple

import numpy as np

import oracle_kinematic as ok

Bar = namedtuple("Bar", ["source", "pairs", "vals", "n_nodes", "truth", "moved", "target"])


def true_dualquats(k, motion=1.0):
    axis = np.array([0.0, 0.2, 1.0])
    return np.array([ok.dq_from_axis_angle(axis, motion * np.deg2rad(2.0) * (i + 1),
                                           motion * (i + 1) * np.array([0.005, 0.0, 0.0075])) for i in range(k)])


def bar_weights(x, k, reverse_every_other=True):
    u = np.clip(x, 0.0, 1.0) * (k - 1)
    a = np.minimum(np.floor(u).astype(np.int64), k - 2)
    u = u - a
    pairs = np.stack([a, a + 1], axis=1).astype(np.int32)
    vals = np.stack([1.0 - u, u], axis=1).astype(np.float32)
    if reverse_every_other:
        pairs[1::2] = pairs[1::2, ::-1]
        vals[1::2] = vals[1::2, ::-1]
    return pairs, vals


def bar(m, k, seed, n=None, motion=1.0, noise=0.002):
    rng = np.random.default_rng(seed)
    centres = rng.uniform([0.0, 0.0, 0.0], [1.0, 0.3, 0.2], size=(60, 3))
    source = centres[rng.integers(0, 60, m)] + 0.015 * rng.normal(size=(m, 3))
    pairs, vals = bar_weights(source[:, 0], k)
    truth = true_dualquats(k, motion)
    moved = ok.skin(truth, pairs, vals, source)
    n = m if n is None else n
    pick = np.arange(m) if n == m else np.sort(rng.choice(m, n, replace=False))
    target = moved[pick] + noise * rng.normal(size=(n, 3))
    return Bar(source, pairs, vals, k, truth, moved, target)


def reference_example():
    """examples/filterreg_deformable.py of the reference: 30 points on a line, 2 nodes, node 1 at 30 deg about z, t = (0, 0, 0.3)."""
    n = 30
    source = np.array([[i * 0.05, 0.0, 0.0] for i in range(n)])
    pairs = np.tile(np.array([0, 1], dtype=np.int32), (n, 1))
    vals = np.array([[float(i) / n, 1.0 - float(i) / n] for i in range(n)], dtype=np.float32)
    truth = np.array([ok.dq_from_axis_angle([0.0, 0.0, 1.0], 0.0, np.zeros(3)),
                      ok.dq_from_axis_angle([0.0, 0.0, 1.0], np.deg2rad(30.0), [0.0, 0.0, 0.3])])
    moved = ok.skin(truth, pairs, vals, source)
    return Bar(source, pairs, vals, 2, truth, moved, moved.copy())


def exact_estep(moved):
    """Exact correspondences: m0 = 1, m1 = the truth."""
    return np.ones(moved.shape[0]), moved.copy(), None


def rms(a, b):
    return float(np.sqrt(np.mean(np.sum(np.square(np.asarray(a) - np.asarray(b)), axis=1))))
