"""Host-side behaviour of the SVR surface (probreg_amd.svm, l2dist_regs): imports, defaults, argument checks.  No GPU."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_imports_without_sklearn_and_without_touching_the_gpu():
    code = (
        "import sys\n"
        "for m in ('sklearn', 'open3d', 'transforms3d', 'six'):\n"
        "    sys.modules[m] = None\n"
        "import probreg_amd\n"
        "from probreg_amd import svm, l2dist_regs, features\n"
        "assert not hasattr(features, 'OneClassSVM') and not hasattr(features, 'FPFH')\n"
        "assert issubclass(svm.OneClassSVM, features.Feature) and l2dist_regs.OneClassSVM is svm.OneClassSVM\n"
        "for n in ('RigidSVR', 'TPSSVR', 'registration_svr', 'L2DistRegistration'):\n"
        "    assert hasattr(l2dist_regs, n)\n"
        "assert svm.working_set_size() >= 2 and svm.working_set_size() % 2 == 0\n"
        "f = svm.OneClassSVM(3, 0.7)\n"
        "f.init(); f.annealing()\n"
        "t = sys.modules.get('torch')\n"
        "assert t is None or not t.cuda.is_initialized()\n"
        "print('ok')\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout


def test_features_module_does_not_carry_the_svm():
    from probreg_amd import features

    assert not hasattr(features, "OneClassSVM")
    assert "OneClassSVM" not in dir(features)


def _defaults(fn):
    return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}


def test_constructor_defaults_match_the_reference():
    from probreg_amd import l2dist_regs, svm

    d = _defaults(svm.OneClassSVM.__init__)
    assert (d["gamma"], d["nu"], d["delta"], d["tol"]) == (0.5, 0.05, 10.0, 1.0e-3)
    assert list(inspect.signature(svm.OneClassSVM.__init__).parameters)[:6] == ["self", "dim", "sigma", "gamma", "nu", "delta"]
    f = svm.OneClassSVM(3, 0.7)
    assert (f._dim, f._sigma, f._gamma, f._nu, f._delta) == (3, 0.7, 0.5, 0.05, 10.0)
    f.annealing()
    assert f._gamma == 5.0 and f._sigma == 0.7
    d = _defaults(l2dist_regs.RigidSVR.__init__)
    assert (d["sigma"], d["delta"], d["gamma"], d["nu"], d["use_estimated_sigma"]) == (1.0, 0.9, 0.5, 0.1, True)
    d = _defaults(l2dist_regs.TPSSVR.__init__)
    assert (d["sigma"], d["delta"], d["gamma"], d["nu"], d["alpha"], d["beta"]) == (1.0, 0.9, 0.5, 0.1, 1.0, 0.1)
    d = _defaults(l2dist_regs.registration_svr)
    assert (d["tf_type_name"], d["maxiter"], d["tol"], d["opt_maxiter"], d["opt_tol"]) == ("rigid", 1, 1.0e-3, 50, 1.0e-3)
    assert list(inspect.signature(l2dist_regs.registration_svr).parameters)[:8] == [
        "source", "target", "tf_type_name", "maxiter", "tol", "opt_maxiter", "opt_tol", "callbacks"]


def test_rigid_svr_hands_the_estimated_sigma_to_the_feature_generator():
    from probreg_amd import l2dist_regs, synthetic

    src = synthetic.surface(100, 0)
    reg = l2dist_regs.RigidSVR(src)  # builds no GPU plan before registration()
    assert reg._feature_gen._sigma == reg._sigma != 1.0
    assert reg._feature_gen._gamma == 1.0 / (2.0 * reg._sigma ** 2)
    assert reg._feature_gen._nu == 0.1
    fixed = l2dist_regs.RigidSVR(src, sigma=0.3, gamma=0.25, use_estimated_sigma=False)
    assert fixed._sigma == 0.3 and fixed._feature_gen._sigma == 0.3 and fixed._feature_gen._gamma == 0.25


def test_unknown_transform_type_raises():
    from probreg_amd import l2dist_regs

    x = np.zeros((10, 3))
    with pytest.raises(ValueError, match="Unknown transform type bogus"):
        l2dist_regs.registration_svr(x, x, "bogus")


def test_shape_checks_need_no_gpu():
    from probreg_amd import svm

    f = svm.OneClassSVM(3, 1.0)
    for bad in (np.zeros((5, 4)), np.zeros(5), np.zeros((5, 1))):
        with pytest.raises(ValueError):
            f.compute(bad)
    with pytest.raises(ValueError):
        f.decision_function(np.zeros((2, 3)))


def test_no_gpu_fails_loudly():
    """Without a GPU the feature generator and the drivers raise instead of computing on the CPU."""
    from probreg_amd import _lib, l2dist_regs, svm, synthetic

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    x = synthetic.surface(40, 0)
    with pytest.raises(_lib.ProbregHipError):
        svm.OneClassSVM(3, 1.0).compute(x)
    with pytest.raises(_lib.ProbregHipError):
        l2dist_regs.registration_svr(x, x + 0.1)
    with pytest.raises(_lib.ProbregHipError):
        l2dist_regs.registration_svr(x, x + 0.1, "nonrigid")
