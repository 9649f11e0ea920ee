"""Host-side behaviour of voxel down-sampling (probreg_amd.preprocess): imports, signatures, argument checks, the ABI's
argument errors.  No GPU."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from probreg_amd import preprocess


def test_imports_without_open3d_and_without_touching_the_gpu():
    code = (
        "import sys\n"
        "for m in ('open3d', 'sklearn'):\n"
        "    sys.modules[m] = None\n"
        "import probreg_amd\n"
        "assert 'preprocess' in probreg_amd._SUBMODULES\n"
        "mod = probreg_amd.preprocess\n"
        "for name in ('voxel_down_sample', 'VoxelPlan', 'VoxelDownSample'):\n"
        "    assert hasattr(mod, name)\n"
        "t = sys.modules.get('torch')\n"
        "assert t is None or not t.cuda.is_initialized()\n"
        "print('ok')\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         universal_newlines=True, env=env, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout


def test_signatures():
    from probreg_amd import global_reg

    sig = inspect.signature(preprocess.voxel_down_sample)
    assert list(sig.parameters) == ["points", "voxel_size", "normals", "attributes", "unit_normals", "device"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [None, None, False, None]
    assert preprocess.VoxelDownSample._fields == ("points", "normals", "attributes", "counts", "first", "inverse")
    for name in ("set_data", "set_channels", "run", "count", "keys", "order", "rows", "means", "channel_means", "counts",
                 "first", "inverse", "close"):
        assert callable(getattr(preprocess.VoxelPlan, name))
    sig = inspect.signature(global_reg.registration_global)
    assert list(sig.parameters)[:6] == ["source", "target", "feature_fn", "max_distance", "mutual", "voxel_size"]
    assert sig.parameters["voxel_size"].default is None
    assert "down-sampled" in global_reg.registration_global.__doc__


class _Cloud(object):
    def __init__(self, points, normals=None):
        self.points = points
        self.normals = normals


def test_bad_arguments_raise_value_error_without_a_gpu():
    ok = np.random.default_rng(0).uniform(size=(6, 3))
    nan, inf = ok.copy(), ok.copy()
    nan[2, 1] = np.nan
    inf[0, 0] = np.inf
    for bad in (np.zeros((5, 1)), np.zeros((5, 4)), np.zeros(6), np.zeros((0, 3)), np.zeros((2, 3, 1)), nan, inf,
                _Cloud(np.zeros((5, 4)))):
        with pytest.raises(ValueError, match="points"):
            preprocess.voxel_down_sample(bad, 0.1)
    for v in (0.0, -0.1, np.nan, np.inf, -np.inf, None, "0.1", np.ones(2)):
        with pytest.raises(ValueError, match="voxel_size"):
            preprocess.voxel_down_sample(ok, v)
    for normals in (np.zeros((5, 3)), np.zeros((6, 2)), np.zeros(6), nan, _Cloud(ok).points[:, :2]):
        with pytest.raises(ValueError, match="normals"):
            preprocess.voxel_down_sample(ok, 0.1, normals=normals)
    with pytest.raises(ValueError, match="normals"):  # a 2-d cloud takes 2-d normals
        preprocess.voxel_down_sample(ok[:, :2], 0.1, normals=ok)
    for attributes in (np.zeros((5, 2)), np.zeros((6, 0)), np.zeros((6, 65)), np.zeros(6), inf):
        with pytest.raises(ValueError, match="attributes"):
            preprocess.voxel_down_sample(ok, 0.1, attributes=attributes)
    # an object's normals are used when they fit the cloud - and are then checked like the argument
    with pytest.raises(ValueError, match="normals"):
        preprocess.voxel_down_sample(_Cloud(ok, nan), 0.1)


def test_registration_global_checks_voxel_size_without_a_gpu():
    from probreg_amd import global_reg

    x = np.random.default_rng(1).uniform(size=(10, 3))
    for v in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="voxel_size"):
            global_reg.registration_global(x, x, voxel_size=v)


def test_sharded_run_is_not_implemented(monkeypatch):
    from probreg_amd import dist, global_reg

    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    x = np.random.default_rng(0).normal(size=(10, 3))
    with pytest.raises(NotImplementedError):
        preprocess.voxel_down_sample(x, 0.1)
    with pytest.raises(NotImplementedError):
        global_reg.registration_global(x, x, voxel_size=0.1)


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "probreg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(prg_voxel_[a-z0-9_]+)\s*\(", text)))


def test_every_voxel_symbol_of_the_header_is_exported():
    from probreg_amd import _lib

    names = _header_symbols()
    assert set(names) >= {"prg_voxel_create", "prg_voxel_destroy", "prg_voxel_set_data", "prg_voxel_set_channels",
                          "prg_voxel_run", "prg_voxel_count", "prg_voxel_get_means", "prg_voxel_get_channel_means",
                          "prg_voxel_get_counts", "prg_voxel_get_first", "prg_voxel_get_inverse", "prg_voxel_get_keys",
                          "prg_voxel_get_order", "prg_voxel_get_rows"}
    for name in names:
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name


def test_abi_argument_checks_need_no_gpu():
    from probreg_amd import _lib

    lib = _lib.lib
    a = np.zeros((4, 3))
    out = np.zeros(12)
    pa, po = _lib.ptr(a), _lib.ptr(out)
    v = ctypes.c_int64(0)
    for fn, args in ((lib.prg_voxel_create, (None, 0, None)), (lib.prg_voxel_set_data, (None, pa, 4, 3)),
                     (lib.prg_voxel_set_channels, (None, pa, 3)), (lib.prg_voxel_run, (None, 0.1)),
                     (lib.prg_voxel_count, (None, ctypes.byref(v))), (lib.prg_voxel_get_means, (None, po)),
                     (lib.prg_voxel_get_channel_means, (None, po)), (lib.prg_voxel_get_counts, (None, po)),
                     (lib.prg_voxel_get_first, (None, po)), (lib.prg_voxel_get_inverse, (None, po)),
                     (lib.prg_voxel_get_keys, (None, po)), (lib.prg_voxel_get_order, (None, po)),
                     (lib.prg_voxel_get_rows, (None, po))):
        assert fn(*args) == _lib.PRG_ERR_INVALID, fn.__name__
        assert "NULL" in _lib.last_error()
    assert lib.prg_voxel_destroy(None) == _lib.PRG_OK
    # the values are checked before the handle is looked at
    for d in (1, 4, 0, -1):
        assert lib.prg_voxel_set_data(None, pa, 4, d) == _lib.PRG_ERR_INVALID
        assert "d must be 2 or 3" in _lib.last_error()
    for n in (0, -1, 1 << 31):
        assert lib.prg_voxel_set_data(None, pa, n, 3) == _lib.PRG_ERR_INVALID
        assert "2^31" in _lib.last_error()
    for c in (-1, 68):
        assert lib.prg_voxel_set_channels(None, pa, c) == _lib.PRG_ERR_INVALID
        assert "0 .. 67" in _lib.last_error()
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.prg_voxel_run(None, size) == _lib.PRG_ERR_INVALID
        assert "voxel_size" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(lib.prg_voxel_run(None, 0.0))


def test_without_a_gpu_the_call_fails_loudly():
    """Without a GPU every entry point raises instead of computing on the CPU (with one, the call answers)."""
    from probreg_amd import _lib, synthetic

    x = synthetic.surface(40, 0)
    if _lib.device_count() > 0:
        assert preprocess.voxel_down_sample(x, 0.2).counts.sum() == 40
        return
    with pytest.raises(_lib.ProbregHipError):
        preprocess.voxel_down_sample(x, 0.2)
    with pytest.raises(_lib.ProbregHipError):
        preprocess.VoxelPlan()
