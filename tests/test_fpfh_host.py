"""Host-side behaviour of the FPFH surface (probreg_amd.fpfh): imports, signature, argument checks.  No GPU."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_imports_without_open3d_and_without_touching_the_gpu():
    code = (
        "import sys\n"
        "for m in ('open3d', 'sklearn', 'six'):\n"
        "    sys.modules[m] = None\n"
        "import probreg_amd\n"
        "from probreg_amd import fpfh, features\n"
        "assert issubclass(fpfh.FPFH, features.Feature) and not hasattr(features, 'FPFH')\n"
        "assert fpfh.max_neighbours() >= 100\n"
        "f = fpfh.FPFH()\n"
        "f.init(); f.annealing()\n"
        "t = sys.modules.get('torch')\n"
        "assert t is None or not t.cuda.is_initialized()\n"
        "print('ok')\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout


def test_features_module_does_not_carry_fpfh():
    from probreg_amd import features

    assert not hasattr(features, "FPFH") and "FPFH" not in dir(features)
    assert "probreg_amd.fpfh" in features.__doc__ and "is not provided" not in features.__doc__


def test_signature_and_defaults_match_the_reference():
    from probreg_amd import features, fpfh

    sig = inspect.signature(fpfh.FPFH.__init__)
    assert list(sig.parameters) == ["self", "radius_normal", "radius_feature", "max_nn_normal", "max_nn_feature", "device"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [0.1, 0.5, 30, 100, None]
    f = fpfh.FPFH(0.2, 0.7)  # the two radii are positional, as in the reference
    assert (f._radius_normal, f._radius_feature, f._max_nn_normal, f._max_nn_feature) == (0.2, 0.7, 30, 100)
    assert isinstance(f, features.Feature) and f.normals_ is None
    for name in ("init", "estimate_normals", "compute", "annealing", "__call__"):
        assert callable(getattr(f, name))


def test_bad_parameters_raise_value_error():
    from probreg_amd import fpfh

    bound = fpfh.max_neighbours()
    for kw in ({"radius_normal": 0.0}, {"radius_normal": -1.0}, {"radius_feature": 0.0}, {"radius_feature": np.nan},
               {"radius_feature": np.inf}, {"max_nn_normal": 0}, {"max_nn_feature": 0}, {"max_nn_feature": -3},
               {"max_nn_normal": bound + 1}, {"max_nn_feature": bound + 1}, {"max_nn_feature": 2.5}):
        with pytest.raises(ValueError):
            fpfh.FPFH(**kw)
    fpfh.FPFH(max_nn_normal=1, max_nn_feature=bound)
    f = fpfh.FPFH()
    f._radius_feature = -0.5  # compute checks again: the parameters may have been changed since the constructor
    with pytest.raises(ValueError):
        f.compute(np.zeros((5, 3)))


def test_bad_data_raises_value_error_without_a_gpu():
    from probreg_amd import fpfh

    f = fpfh.FPFH()
    nan = np.zeros((5, 3))
    nan[2, 1] = np.nan
    inf = np.zeros((5, 3))
    inf[0, 0] = np.inf
    for bad in (np.zeros((5, 2)), np.zeros((5, 4)), np.zeros(6), np.zeros((0, 3)), np.zeros((2, 3, 1)), nan, inf):
        with pytest.raises(ValueError):
            f.compute(bad)
        with pytest.raises(ValueError):
            f.estimate_normals(bad)


def test_abi_argument_checks_need_no_gpu():
    import ctypes

    from probreg_amd import _lib

    k = ctypes.c_int(0)
    assert _lib.lib.prg_fpfh_max_nn(ctypes.byref(k)) == _lib.PRG_OK and k.value >= 100
    assert _lib.lib.prg_fpfh_max_nn(None) == _lib.PRG_ERR_INVALID
    for fn, args in ((_lib.lib.prg_fpfh_search, (None, 0, 0.1, 30)), (_lib.lib.prg_fpfh_normals, (None,)),
                     (_lib.lib.prg_fpfh_spfh, (None,)), (_lib.lib.prg_fpfh_fpfh, (None,)),
                     (_lib.lib.prg_fpfh_set_data, (None, None, 3)), (_lib.lib.prg_fpfh_get_fpfh, (None, None))):
        assert fn(*args) == _lib.PRG_ERR_INVALID
        assert "NULL" in _lib.last_error()


def test_no_gpu_fails_loudly():
    """Without a GPU the descriptor and the registration that uses it raise instead of computing on the CPU."""
    from probreg_amd import _lib, filterreg, fpfh, synthetic

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    x = synthetic.surface(40, 0)
    with pytest.raises(_lib.ProbregHipError):
        fpfh.FPFH().compute(x)
    with pytest.raises(_lib.ProbregHipError):
        fpfh.FPFH().estimate_normals(x)
    with pytest.raises(_lib.ProbregHipError):
        fpfh.FpfhPlan()
    with pytest.raises(_lib.ProbregHipError):
        filterreg.registration_filterreg(x, x + 0.1, sigma2=1000, feature_fn=fpfh.FPFH(0.15, 0.3))
