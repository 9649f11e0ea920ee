"""The NumPy restatement of DESIGN.md section 3.10 (tests/oracle_kinematic.py) against the reference's own code on the
reference's example, and the recorded reasons why the default M-step is the complete Gauss-Newton system and not the
reference's.  No GPU."""
import os

import numpy as np
import pytest

import kinematic_cases as kc
import oracle_kinematic as ok
from conftest import GOLDEN_DIR, Golden, rel_err


@pytest.fixture(scope="module")
def example():
    return Golden(os.path.join(GOLDEN_DIR, "kinematic_golden.npz")).case("example")


def _max_err(a, b):
    return float(np.max(np.linalg.norm(np.asarray(a) - np.asarray(b), axis=1)))


def test_skinning_reproduces_the_reference_on_its_example(example):
    """What the fixture pins down: the reference's own CALL STRUCTURE (which dual quaternions are blended with which
    weights, `op.dlb` per point, `transform_point`; in the M-step test below its loops, matrix and gradient).  What it
    does not: the dual-quaternion conventions themselves.  `dq3d` could not be run, so the stand-in the reference was
    executed with (tests/dq3d_standin.py) takes its quaternion algebra from this very restatement - for the
    conventions the comparison is circular, and DESIGN.md section 3.10 is their only definition.  The conventions are
    checked independently below against rotation matrices, and on the GPU by kernels that use another formulation."""
    out = ok.skin(example["dualquats"], example["pairs"], example["vals"], example["source"])
    assert rel_err(out, example["transformed"]) < 1e-12
    case = kc.reference_example()
    assert rel_err(case.moved, example["transformed"]) < 1e-12


def test_reference_form_reproduces_the_reference_mstep(example):
    """Both sides are fp64 NumPy with the same algebra and cond(A) ~ 6e3: 1e-9 relative leaves orders of magnitude."""
    src, moved = example["source"], example["transformed"]
    res = ok.maximization_step(src, moved.shape[0], np.ones(src.shape[0]), moved, None, np.tile(np.eye(1, 8)[0], (2, 1)),
                               example["pairs"], example["vals"], 0.01, reference_form=True)
    print("dualquats", rel_err(res.dualquats, example["mstep_dualquats"]), "q", res.q, example["mstep_q"])
    assert rel_err(res.dualquats, example["mstep_dualquats"]) < 1e-9
    assert abs(res.q - example["mstep_q"]) <= 1e-9 * abs(example["mstep_q"])
    out = ok.skin(res.dualquats, example["pairs"], example["vals"], src)
    assert rel_err(out, example["mstep_transformed"]) < 1e-9
    assert res.sigma2 == example["mstep_sigma2"] == 0.01


@pytest.mark.parametrize("m,k", [(200, 2), (300, 3), (2000, 8)])
def test_complete_form_recovers_the_truth_on_exact_correspondences(m, k):
    """Motion 4x the bar's; the answer is within the inner stop tolerance 1e-4 of the truth (measured: 7.3e-7, 1.0e-5
    and 3.0e-5, in 5, 6 and 32 inner iterations)."""
    case = kc.bar(m, k, seed=11 + k, motion=4.0)
    m0, m1, _ = kc.exact_estep(case.moved)
    res = ok.maximization_step(case.source, m, m0, m1, None, np.tile(np.eye(1, 8)[0], (k, 1)), case.pairs, case.vals, 1e-3)
    err = _max_err(ok.skin(res.dualquats, case.pairs, case.vals, case.source), case.moved)
    print("(M, K) = (%d, %d): %d inner iterations, max error %.3g" % (m, k, res.n_iter, err))
    assert err < 1e-4
    assert res.n_iter < 50


def test_reference_form_fails_on_three_nodes_and_works_on_its_example():
    """The recorded reason for the deviation: the reference's system only solves its own example."""
    case = kc.bar(300, 3, seed=14, motion=4.0)
    m0, m1, _ = kc.exact_estep(case.moved)
    res = ok.maximization_step(case.source, 300, m0, m1, None, np.tile(np.eye(1, 8)[0], (3, 1)), case.pairs, case.vals, 1e-3,
                               reference_form=True)
    start = _max_err(case.source, case.moved)
    out = ok.skin(res.dualquats, case.pairs, case.vals, case.source)
    end = _max_err(out, case.moved) if np.isfinite(out).all() else np.inf
    print("3 nodes, reference form: max error %.3g -> %.3g" % (start, end))
    assert end > start
    ex = kc.reference_example()
    m0, m1, _ = kc.exact_estep(ex.moved)
    res = ok.maximization_step(ex.source, 30, m0, m1, None, np.tile(np.eye(1, 8)[0], (2, 1)), ex.pairs, ex.vals, 0.01,
                               reference_form=True)
    err = _max_err(ok.skin(res.dualquats, ex.pairs, ex.vals, ex.source), ex.moved)
    print("the reference's example, reference form: max error %.3g" % err)
    assert err < 1e-5


def test_zero_m0_points_are_ignored_by_default_and_fatal_in_reference_form():
    """filterreg.py:223 turns m0 == 0 into float32 eps: at w = 0 such a point is pulled to the origin with full weight.
    The points zeroed here are the four at the far end of the line - the fringe is where a lattice finds no target, and
    the origin is farthest from them."""
    ex = kc.reference_example()
    m0, m1, _ = kc.exact_estep(ex.moved)
    dead = np.zeros(30, dtype=bool)
    dead[[26, 27, 28, 29]] = True
    m0z, m1z = m0.copy(), m1.copy()
    m0z[dead], m1z[dead] = 0.0, 0.0
    ident = np.tile(np.eye(1, 8)[0], (2, 1))
    full = ok.maximization_step(ex.source, 30, m0z, m1z, None, ident, ex.pairs, ex.vals, 0.01)
    keep = ~dead
    # (n_target / m only enters through c, which is 0 at w = 0)
    cut = ok.maximization_step(ex.source[keep], 30, m0[keep], m1[keep], None, ident, ex.pairs[keep], ex.vals[keep], 0.01)
    assert full.n_iter == cut.n_iter
    assert rel_err(full.dualquats, cut.dualquats) < 1e-12
    assert abs(full.q - cut.q) <= 1e-12 * max(abs(cut.q), 1e-300) + 1e-300
    ref = ok.maximization_step(ex.source, 30, m0z, m1z, None, ident, ex.pairs, ex.vals, 0.01, reference_form=True)
    out = ok.skin(ref.dualquats, ex.pairs, ex.vals, ex.source)
    extent = float(np.max(np.abs(ex.moved - ex.moved.mean(0))))
    moved_by = _max_err(out, ex.moved) if np.isfinite(out).all() else np.inf
    print("reference form with 4 zero m0: moved by %.3g (extent %.3g)" % (moved_by, extent))
    assert moved_by > extent


def test_conventions_agree_with_rotation_matrices():
    """Independent of the quaternion algebra: a node's dual quaternion from (axis, angle, t) moves points as R x + t with
    R from Rodrigues' formula, and a product moves them as the composition (b first)."""
    rng = np.random.default_rng(2)
    pts = rng.normal(size=(20, 3))

    def rodrigues(axis, ang):
        axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
        kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.identity(3) + np.sin(ang) * kx + (1.0 - np.cos(ang)) * kx @ kx

    ax_a, an_a, t_a = rng.normal(size=3), 0.7, rng.normal(size=3)
    ax_b, an_b, t_b = rng.normal(size=3), 2.9, rng.normal(size=3)
    qa, qb = ok.dq_from_axis_angle(ax_a, an_a, t_a), ok.dq_from_axis_angle(ax_b, an_b, t_b)
    ra, rb = rodrigues(ax_a, an_a), rodrigues(ax_b, an_b)
    assert np.max(np.abs(ok.dq_transform(qa[None], pts) - (pts @ ra.T + t_a))) < 1e-14
    both = ok.dq_transform(ok.dq_mul(qa, qb)[None], pts)
    assert np.max(np.abs(both - ((pts @ rb.T + t_b) @ ra.T + t_a))) < 1e-13
    tw = np.r_[an_a * ax_a / np.linalg.norm(ax_a), t_a]
    assert np.max(np.abs(ok.dq_from_twist(tw) - qa)) < 1e-15
