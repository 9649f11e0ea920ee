"""Host-side pieces of GMMReg (no GPU): quaternion algebra, the thin-plate-spline kernel and basis, the import surface,
and - where the reference tree and scikit-learn are present - that tests/golden/make_gmmreg_golden.py reproduces the
committed fixture."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR, ROOT, Golden


@pytest.fixture(scope="module")
def golden():
    return Golden(os.path.join(GOLDEN_DIR, "gmmreg_golden.npz"))


def test_diff_rot_from_quaternion_against_central_differences():
    """dR/dq matches central differences of quat2mat, on and off the unit sphere."""
    from probreg_amd import se3_op

    rng = np.random.default_rng(0)
    h = 1.0e-6
    for trial in range(10):
        q = rng.normal(size=4)
        if trial % 2:
            q /= np.linalg.norm(q)
        d = se3_op.diff_rot_from_quaternion(q)
        assert d.shape == (4, 3, 3)
        for i in range(4):
            e = np.zeros(4)
            e[i] = h
            num = (se3_op.quat2mat(q + e) - se3_op.quat2mat(q - e)) / (2.0 * h)
            assert np.max(np.abs(d[i] - num)) < 1e-8


def test_quat2mat_convention(golden):
    from probreg_amd import se3_op

    case = golden.case("cost/quat")
    for q, rot in zip(case["q"], case["rot"]):
        assert np.max(np.abs(se3_op.quat2mat(q) - rot)) < 1e-15
    r = se3_op.quat2mat([0.3, -0.5, 0.2, 0.7])  # not a unit quaternion: normalised implicitly
    assert np.allclose(r @ r.T, np.identity(3), atol=1e-14) and abs(np.linalg.det(r) - 1.0) < 1e-14
    assert np.array_equal(se3_op.quat2mat([1e-9, 0.0, 0.0, 0.0]), np.identity(3))
    # reference_form=True is the reference's function entry by entry (what its BFGS runs differentiate with); it
    # is the derivative at the identity and not at a general quaternion
    for q, d in zip(case["q"][:3], case["d_rot"]):
        assert np.max(np.abs(se3_op.diff_rot_from_quaternion(q, reference_form=True) - d)) < 1e-14
    exact = se3_op.diff_rot_from_quaternion(case["q"][0])
    assert np.max(np.abs(exact - case["d_rot"][0])) < 1e-15
    assert np.max(np.abs(se3_op.diff_rot_from_quaternion(case["q"][1]) - case["d_rot"][1])) > 0.1


@pytest.mark.parametrize("name", ["tps3", "tps2"])
def test_tps_kernel_and_prepare(golden, name):
    from probreg_amd import math_utils as mu
    from probreg_amd import transformation as tf

    case = golden.case("cost/" + name)
    ctrl = case["mu_source"]
    dim = ctrl.shape[1]
    k = mu.tps_kernel(ctrl, ctrl)
    assert k.dtype == np.float32 and k.shape == (ctrl.shape[0],) * 2
    assert np.max(np.abs(k - case["tps_kernel"])) <= 1e-6 * np.max(np.abs(case["tps_kernel"]))
    assert np.all(np.diag(k) == 0.0)
    a = np.r_[np.zeros((1, dim)), np.identity(dim)]
    v = np.zeros((ctrl.shape[0] - dim - 1, dim))
    tps = tf.TPSTransformation(a, v, ctrl)
    basis, kernel = tps.prepare(ctrl)
    assert np.max(np.abs(basis - case["basis"])) <= 1e-9 * np.max(np.abs(case["basis"]))
    assert np.max(np.abs(kernel - case["kernel"])) <= 1e-9 * np.max(np.abs(case["kernel"]))
    assert np.allclose(tps.transform(ctrl), ctrl, atol=1e-12)  # identity affine part, no warp
    with pytest.raises(ValueError):
        mu.tps_kernel(np.zeros((3, 4)), np.zeros((3, 4)))


def test_tps_kernel_values():
    from probreg_amd import math_utils as mu

    x2 = np.array([[0.0, 0.0], [3.0, 4.0], [1e-6, 0.0]])
    k2 = mu.tps_kernel(x2, x2[:1])
    assert abs(k2[1, 0] - 25.0 * np.log(5.0)) < 1e-4 and k2[0, 0] == 0.0 and k2[2, 0] == 0.0  # r^2 <= 1e-9 -> 0
    x3 = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]])
    assert abs(mu.tps_kernel(x3, x3)[0, 1] + 3.0) < 1e-6


def test_imports_without_sklearn_and_without_touching_the_gpu():
    code = (
        "import sys\n"
        "for m in ('sklearn', 'open3d', 'transforms3d', 'six'):\n"
        "    sys.modules[m] = None\n"
        "import probreg_amd\n"
        "from probreg_amd import l2dist_regs, features, cost_functions, se3_op\n"
        "assert probreg_amd.l2dist_regs is l2dist_regs and probreg_amd.features is features\n"
        "assert callable(l2dist_regs.registration_gmmreg)\n"
        "for n in ('Feature', 'GMM'):\n"
        "    assert hasattr(features, n)\n"
        "for n in ('FPFH', 'OneClassSVM'):\n"
        "    assert not hasattr(features, n)\n"
        "for n in ('CostFunction', 'RigidCostFunction', 'TPSCostFunction', 'compute_l2_dist'):\n"
        "    assert hasattr(cost_functions, n)\n"
        "for n in ('L2DistRegistration', 'RigidGMMReg', 'TPSGMMReg'):\n"
        "    assert hasattr(l2dist_regs, n)\n"
        "g = features.GMM()\n"
        "assert g._n_gmm_components == 800\n"
        "t = sys.modules.get('torch')\n"
        "assert t is None or not t.cuda.is_initialized()\n"
        "print('ok')\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout


def test_gmm_argument_checks_need_no_gpu():
    from probreg_amd import features

    with pytest.raises(ValueError):
        features.GMM(0)
    with pytest.raises(ValueError):
        features.GMM(10, means_init=np.zeros((10, 3)))
    with pytest.raises(ValueError):
        features.GMM(10).compute(np.zeros((5, 3)))  # K > N, before any device work
    with pytest.raises(ValueError):
        features.GMM(2).compute(np.zeros((5, 4)))
    assert features.seed_trials(800) == 2 + int(np.log(800))
    u = features.seed_uniforms(50, 7)
    assert u.shape == (50, features.seed_trials(50)) and np.array_equal(u, features.seed_uniforms(50, 7))
    assert np.all((u >= 0.0) & (u < 1.0))


def test_fixture_em_cases_rederive_from_sklearn(golden):
    """The generator is reproducible: scikit-learn, run again on the stored inputs, returns the stored results."""
    sklearn = pytest.importorskip("sklearn")
    del sklearn
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_gmmreg_golden as mk
    finally:
        sys.path.pop(0)
    for name in ("bunny_k32", "fish_k32", "surface5k_k100", "surface5k_far"):
        case = golden.case("em/" + name)
        spec = [str(s) for s in case["spec"]]
        x = mk.cloud_from_spec(spec, case.get("x"))
        k = int(case["k"])
        mu0 = x[case["init_idx"]].copy()
        mu0[0] = case["init_mean0"]
        gm = mk.sk_fit(x, np.full(k, 1.0 / k), mu0, np.full(k, float(case["init_precision"])), int(case["max_iter"]))
        assert gm.n_iter_ == int(case["n_iter"])
        for key in ("weights", "means", "covariances"):
            ref = case[key]
            assert np.max(np.abs(getattr(gm, key + "_") - ref)) <= 1e-12 * np.max(np.abs(ref)), (name, key)
        assert np.max(np.abs(np.array(gm.lower_bounds_) - case["lower_bounds"])) < 1e-12
