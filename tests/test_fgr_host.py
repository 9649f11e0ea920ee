"""The definitions of fast global registration (csrc/fgr.h: the normalised point, the edge test of a trial, the line-process
weight, what a pair adds to the 27 sums and to the objective, the schedule of mu, the way back to the caller's units - what
the kernels of csrc/fgr.hip compute by) on the host: tests/host/fgr_check.cpp drives the header over cases of
tests/fgr_cases.py and prints means, scale, the accepted tuples, the trial count, the 28 sums, the weights, the sequence of
mu and the final pose as hex floats; every one of them must equal tests/oracle_fgr.py bit for bit.  It is built with the host
C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically) with -ffp-contract=off, as the header
asks, not linked against the HIP runtime, and run as a program of its own.  No GPU.

Plus the host-side behaviour of ``global_reg.registration_fgr``: argument checks, the no-GPU error."""
import os
import subprocess

import numpy as np
import pytest

import fgr_cases as fc
import oracle_fgr as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def _hex(v):
    return " ".join(float(x).hex() for x in v)


def _cases():
    """name -> (source, target, corr, keywords of of.fgr)"""
    small = fc.case(600, 0.5, 0)
    limit = fc.case(1000, 0.8, 0)   # the trial limit ends the search
    exact = fc.exact_case()
    rng = np.random.default_rng(4)
    return [("wrong50", small[0], small[1], small[2], dict(seed=0)),
            ("limit", limit[0], limit[1], limit[2], dict(seed=0)),
            ("cap7", small[0], small[1], small[2][:60], dict(seed=2 ** 63 + 5, maximum_tuple_count=7, tuple_scale=0.9)),
            ("all_pairs", small[0][:130], small[1][:200], np.stack([rng.integers(0, 130, 193), rng.integers(0, 200, 193)], 1),
             dict(tuple_test=False, iteration_number=9, division_factor=2.0)),
            ("absolute", exact[0] * 3.0 + 2.0 ** 20, exact[1] * 3.0, exact[2],
             dict(use_absolute_scale=True, maximum_correspondence_distance=0.3, iteration_number=24, decrease_mu=True)),
            ("no_decrease", exact[0], exact[1], exact[2], dict(decrease_mu=False, iteration_number=6))]


def _write(path, src, tgt, corr, ref, kw):
    with open(path, "w") as f:
        f.write("%d %d %d %d %s %d %d %d %d %d %s %s %s\n" % (
            src.shape[0], tgt.shape[0], corr.shape[0], kw.get("seed", 0), float(kw.get("tuple_scale", 0.95)).hex(),
            kw.get("maximum_tuple_count", 1000), int(kw.get("use_absolute_scale", False)), int(kw.get("tuple_test", True)),
            kw.get("iteration_number", 64), int(kw.get("decrease_mu", True)), float(kw.get("division_factor", 1.4)).hex(),
            float(kw.get("maximum_correspondence_distance", 0.025)).hex(), float(ref["mu"]).hex()))
        f.write(_hex(ref["pose"]) + "\n")
        for rows in (src, tgt):
            for r in rows:
                f.write(_hex(r) + "\n")
        for r in corr:
            f.write("%d %d\n" % (r[0], r[1]))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fgr") / "fgr_check")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
           "-fno-sanitize-recover=undefined,float-cast-overflow", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "fgr_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    return exe


def test_header_equals_the_restatement_bit_for_bit(program, tmp_path):
    cases, refs, paths = _cases(), [], []
    for name, src, tgt, corr, kw in cases:
        refs.append(of.fgr(src, tgt, corr, **kw))
        paths.append(str(tmp_path / (name + ".txt")))
        _write(paths[-1], src, tgt, corr, refs[-1], kw)
    run = subprocess.run([program] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "fgr_check ok" and len(lines) == 7 * len(cases) + 1
    for k, ((name, src, tgt, corr, kw), ref) in enumerate(zip(cases, refs)):
        mus, pose = lines[7 * k + 5].split(), lines[7 * k + 6].split()
        rows = {ln.split()[0]: ln.split()[1:] for ln in lines[7 * k:7 * k + 5]}
        want = np.concatenate([ref["mean_p"], ref["mean_q"], [ref["scale"]]])
        assert np.array_equal(_bits([float.fromhex(v) for v in rows["norm"]]), _bits(want)), name
        assert [int(v) for v in rows["tuples"]] == [ref["n_tuples"], ref["n_trials"]], name
        assert np.array_equal(np.array([int(v) for v in rows["used"]], dtype=np.int64), ref["used"]), name
        ref_sums = of.sums(ref["up"], ref["uq"], ref["pose"], ref["mu"])
        assert np.array_equal(_bits([float.fromhex(v) for v in rows["sums"]]), _bits(ref_sums)), name
        assert np.array_equal(_bits([float.fromhex(v) for v in rows["weights"]]), _bits(ref["weights"])), name
        assert mus[0] == "mu" and pose[0] == "pose"
        assert ref["n_iter"] == kw.get("iteration_number", 64), name
        assert np.array_equal(_bits([float.fromhex(v) for v in mus[1:]]), _bits(ref["mus"])), name
        assert np.array_equal(_bits([float.fromhex(v) for v in pose[1:]]), _bits(ref["pose_out"])), name
    assert refs[1]["n_trials"] == 100 * 1000 and refs[1]["n_tuples"] < 1000   # the limit case is one
    assert refs[2]["n_tuples"] == 7 and refs[2]["n_trials"] < 100 * 60


def test_interface_and_argument_checks_need_no_gpu(monkeypatch):
    import inspect

    from probreg_amd import dist, global_reg as gr

    assert gr.FgrResult._fields == ("transformation", "fitness", "inlier_rmse", "inliers", "used", "weights", "mu", "n_iter",
                                    "n_tuples", "n_trials", "status")
    sig = inspect.signature(gr.registration_fgr)
    assert list(sig.parameters) == ["source", "target", "correspondences", "maximum_correspondence_distance", "iteration_number",
                                    "division_factor", "decrease_mu", "use_absolute_scale", "tuple_test", "tuple_scale",
                                    "maximum_tuple_count", "seed", "max_distance", "device"]
    defaults = [sig.parameters[k].default for k in list(sig.parameters)[3:]]
    assert defaults == [0.025, 64, 1.4, True, False, True, 0.95, 1000, 0, None, None]
    assert inspect.signature(gr.registration_global).parameters["method"].default == "ransac"
    for name in ("set_clouds", "set_correspondences", "normalise", "tuples", "set_used", "sums", "step", "iterate", "weights"):
        assert callable(getattr(gr.FgrPlan, name))
    src, tgt, corr, _, _ = fc.exact_case()
    nan = src.copy()
    nan[3, 1] = np.nan
    far = corr.copy()
    far[5, 1] = tgt.shape[0]
    neg = corr.copy()
    neg[0, 0] = -1
    bad = [dict(source=src[:, :2]), dict(source=nan), dict(target=np.zeros((0, 3))), dict(correspondences=corr[:2]),
           dict(correspondences=corr.astype(np.float64)), dict(correspondences=corr[:, :1]), dict(correspondences=far),
           dict(correspondences=neg), dict(tuple_scale=0.0), dict(tuple_scale=1.5), dict(tuple_scale=np.nan),
           dict(division_factor=1.0), dict(division_factor=np.inf), dict(iteration_number=-1), dict(iteration_number=2.5),
           dict(maximum_tuple_count=0), dict(maximum_tuple_count=1.5), dict(maximum_correspondence_distance=-1.0),
           dict(maximum_correspondence_distance=np.nan), dict(max_distance=-0.1), dict(max_distance=np.inf)]
    for kw in bad:
        args = dict(source=src, target=tgt, correspondences=corr)
        args.update(kw)
        with pytest.raises(ValueError):
            gr.registration_fgr(**args)
    big = np.lib.stride_tricks.as_strided(corr, shape=(gr.FGR_MAX_CORRESPONDENCES + 1, 2), strides=(0, corr.strides[1]))
    with pytest.raises(ValueError, match="at most"):
        gr.registration_fgr(src, tgt, big)
    with pytest.raises(ValueError, match="method"):
        gr.registration_global(src, tgt, method="teaser")
    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        gr.registration_fgr(src, tgt, corr)


def test_abi_argument_checks_need_no_gpu():
    import ctypes

    from probreg_amd import _lib

    lib = _lib.lib
    a = np.zeros((4, 3))
    pa = _lib.ptr(a)
    n64, st, d = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0.0)
    for fn, args in ((lib.prg_fgr_create, (None, 0, None)), (lib.prg_fgr_set_clouds, (None, pa, 4, pa, 4)),
                     (lib.prg_fgr_set_correspondences, (None, pa, 4)), (lib.prg_fgr_normalise, (None, 0, pa, pa, ctypes.byref(d))),
                     (lib.prg_fgr_set_chunk, (None, 0)),
                     (lib.prg_fgr_tuples, (None, 0, 0.95, 10, ctypes.byref(n64), ctypes.byref(n64))),
                     (lib.prg_fgr_set_used, (None, pa, 4)), (lib.prg_fgr_get_used, (None, pa)),
                     (lib.prg_fgr_set_state, (None, pa, 1.0)), (lib.prg_fgr_sums, (None, pa)),
                     (lib.prg_fgr_step, (None, 1, 1.4, 0.025)), (lib.prg_fgr_iterate, (None, 4, 1, 1.4, 0.025)),
                     (lib.prg_fgr_get_state, (None, 0, pa, ctypes.byref(d), ctypes.byref(n64), ctypes.byref(st), ctypes.byref(d))),
                     (lib.prg_fgr_get_weights, (None, pa))):
        assert fn(*args) == _lib.PRG_ERR_INVALID
        assert "NULL" in _lib.last_error()
    assert lib.prg_fgr_destroy(None) == _lib.PRG_OK


def test_no_gpu_fails_loudly():
    """Without a GPU the entry points raise instead of computing on the CPU."""
    from probreg_amd import _lib, global_reg as gr

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    src, tgt, corr, _, _ = fc.exact_case()
    with pytest.raises(_lib.ProbregHipError):
        gr.FgrPlan()
    with pytest.raises(_lib.ProbregHipError):
        gr.registration_fgr(src, tgt, corr)
