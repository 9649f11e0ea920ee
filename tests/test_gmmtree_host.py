"""GMMTree without a GPU: the fp64 restatement (tests/oracle_gmmtree.py) against an independent EM implementation and
the committed reference fixtures, and the product's Python driver (probreg_amd.gmmtree) run on the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT

import oracle_gmmtree as og

GOLDEN = os.path.join(GOLDEN_DIR, "gmmtree_golden.npz")
DRIVER_CASES = ["bunny_L1", "bunny_L2", "tiny40_L2", "bunny_scale_L2", "planar_L2", "rankdef_L2"]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def case(z, name):
    p = name + "/"
    c = {k[len(p):]: z[k] for k in z.files if k.startswith(p)}
    if "tgt" not in c:
        c["tgt"] = c["src"] @ c["tgt_rot"].T + c["tgt_t"]
    return c


def test_level_one_is_one_em_update_of_sklearn_gaussian_mixture():
    """One build EM iteration at L = 1 (8 full-covariance components, no parent) equals one EM update of sklearn's
    GaussianMixture started from the same weights, means and precisions (reg_covar = 0)."""
    mixture = pytest.importorskip("sklearn.mixture")
    from probreg_amd import synthetic

    x = synthetic.surface(3000, 5)
    idx = og.init_indices(x.shape[0], 1, seed=2)
    nodes0 = og.init_nodes(x, 1, idx)
    nodes1, info = og.build(x, 1, idx, lambda_s=1e30, max_iter=1)  # exactly one E + M
    assert info["iters"] == [1]
    sig0 = nodes0[:, 4:][:, og.SYM]
    gm = mixture.GaussianMixture(8, covariance_type="full", reg_covar=0.0, max_iter=1, tol=0.0,
                                 weights_init=nodes0[:, 0], means_init=nodes0[:, 1:4],
                                 precisions_init=np.linalg.inv(sig0))
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit(x)
    np.testing.assert_allclose(nodes1[:, 0], gm.weights_, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(nodes1[:, 1:4], gm.means_, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(nodes1[:, 4:][:, og.SYM], gm.covariances_, rtol=1e-8, atol=1e-12)


def test_restatement_reproduces_the_committed_fixture_nodes(golden):
    """The restatement alone (no reference code) rebuilds the fixture trees and E-step moments."""
    for name in ("bunny_L2", "tiny40_L2"):
        c = case(golden, name)
        lv = int(c["tree_level"])
        nodes, info = og.build(c["src"], lv, c["idx"], float(c["lambda_s"]))
        assert info["iters"] == list(c["iters"])
        np.testing.assert_array_equal(nodes, c["nodes"])
        x = c["tgt"] @ c["e1_rot"].T + c["e1_t"]
        m0, m1, m2 = og.reg_estep(x, c["nodes"], lv, float(c["lambda_c"]))
        np.testing.assert_allclose(m0, c["e1_m0"], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(m1, c["e1_m1"], rtol=1e-12, atol=1e-12)


def test_fixture_has_no_near_ties(golden):
    """Stop decisions and argmax choices in the fixtures are far from ties, so fp64 rounding cannot flip them.  (A build
    gap of 0 is an exact tie between identical nodes - two leaves started from the same point - which every
    implementation breaks toward the lower index.)"""
    names = sorted({k.split("/")[0] for k in golden.files})
    for name in names:
        c = case(golden, name)
        lam_s = float(c["lambda_s"])
        dq = c["dq_last2"]
        assert np.all(dq[:, 0] < lam_s * 0.999) and np.all(dq[:, 1] > lam_s * 1.0001), name
        assert float(c["e0_gap"]) > 1e-7 and float(c["e1_gap"]) > 1e-7, name


@pytest.mark.skipif(not os.path.isfile("/root/reference/probreg/gmmtree.py"), reason="reference tree not present")
def test_regenerating_a_small_fixture_reproduces_the_npz(tmp_path, golden):
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r);"
            "import make_gmmtree_golden as g; d = g.main(('bunny_L1',)); np.savez(%r, **d)"
            % (ROOT, os.path.join(ROOT, "tests", "golden"), str(tmp_path / "g.npz")))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, stdout=subprocess.DEVNULL)
    z = np.load(str(tmp_path / "g.npz"))
    for k in z.files:
        a, b = z[k], golden[k]
        if a.dtype.kind in "fc":
            np.testing.assert_array_equal(a, b, err_msg=k)
        else:
            assert np.array_equal(a, b), k


@pytest.fixture
def oracle_plan(monkeypatch):
    from probreg_amd import gmmtree

    monkeypatch.setattr(gmmtree, "GmmTreePlan", og.OracleGmmTreePlan)
    return gmmtree


@pytest.mark.parametrize("name", DRIVER_CASES)
def test_driver_on_the_restatement_matches_the_reference_driver(oracle_plan, golden, name):
    gmmtree = oracle_plan
    c = case(golden, name)
    kw = dict(tree_level=int(c["tree_level"]), lambda_c=float(c["lambda_c"]), lambda_s=float(c["lambda_s"]),
              tf_init_params=dict(rot=c["init_rot"], t=c["init_t"], scale=float(c["init_scale"])))
    seen = []
    cb = [lambda tr: seen.append((tr.rot.copy(), tr.t.copy(), tr.scale))]
    if str(c["raises"]):
        with pytest.raises(ValueError):
            gmmtree.registration_gmmtree(c["src"], c["tgt"], callbacks=cb, **kw)
    else:
        res = gmmtree.registration_gmmtree(c["src"], c["tgt"], callbacks=cb, **kw)
        np.testing.assert_allclose(res.transformation.rot, c["rot"], atol=1e-12)
        np.testing.assert_allclose(res.transformation.t, c["t"], atol=1e-12)
        np.testing.assert_allclose(res.q, c["q"], rtol=1e-10, atol=1e-20)
    # the callbacks got tf.inverse() of every iteration
    assert len(seen) == int(c["n_iter"])
    for k, (r, t, s) in enumerate(seen):
        np.testing.assert_allclose(r, c["cb_rot"][k], atol=1e-12)
        np.testing.assert_allclose(t, c["cb_t"][k], atol=1e-12)


def test_driver_estep_and_mstep_on_the_restatement(oracle_plan, golden):
    gmmtree = oracle_plan
    from probreg_amd import transformation as tf

    c = case(golden, "bunny_L2")
    g = gmmtree.GMMTree(tree_level=2)
    g.set_nodes(og.nodes_as_tuples(c["nodes"]))
    np.testing.assert_array_equal(np.array([n[0] for n in g._nodes]), c["nodes"][:, 0])
    trans = tf.RigidTransformation(c["e1_rot"], c["e1_t"])
    est = g.expectation_step(trans.transform(c["tgt"]))
    assert len(est.moments) == c["nodes"].shape[0]
    np.testing.assert_allclose([m[0] for m in est.moments], c["e1_m0"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(np.array([m[2] for m in est.moments]), c["e1_m2"], rtol=1e-12, atol=1e-14)
    ms = g.maximization_step(est, trans)
    np.testing.assert_allclose(ms.transformation.rot, c["e1_mrot"], atol=1e-12)
    np.testing.assert_allclose(ms.transformation.t, c["e1_mt"], atol=1e-12)
    np.testing.assert_allclose(ms.q, c["e1_mq"], rtol=1e-10)


def test_tree_level_out_of_range_raises():
    from probreg_amd import gmmtree

    for lv in (0, 5, 2.0):
        with pytest.raises(ValueError):
            gmmtree.GMMTree(tree_level=lv)
