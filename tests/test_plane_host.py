"""The decisions of plane segmentation (csrc/plane_seg.h: the draw, the validity test, the plane of a triple, the sign rule, the
anchored distance, the inlier predicate, the ranking, the refit's covariance - what the kernels of csrc/plane_seg.hip decide
by) on the host: tests/host/plane_seg_check.cpp drives the header over the exact clouds of tests/plane_cases.py, the fixed
300-point cloud, its exact shift, and the table scene with its normals, and prints triples, flags, planes, counts, sums, the
winner and one refit's sums and covariance as hex floats; every one of them must equal tests/oracle_plane.py bit for bit.
It is built with the host C++ compiler under AddressSanitizer and UBSan (their runtimes linked in statically) with
-ffp-contract=off, as the header asks, not linked against the HIP runtime, and run as a program of its own.  No GPU.

Plus the host-side behaviour of ``preprocess.segment_plane`` / ``segment_planes``: argument checks, the no-GPU error."""
import os
import subprocess

import numpy as np
import pytest

import oracle_plane as op
import plane_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def _cases():
    pts, nrm, _, _ = pc.table_scene()
    return [("lattices", pc.lattices(), None, 64, 0, 0, 0.0, None),
            ("quarter", pc.quarter_cloud(), None, 64, 0, 0, 0.25, None),
            ("collinear", pc.collinear_cloud(), None, 64, 0, 0, 0.1, None),
            ("grid", pc.grid_cloud(), None, pc.GRID_HYP, pc.GRID_SEED, 0, pc.GRID_TAU, None),
            ("grid_shifted", pc.grid_cloud() + pc.SHIFT_EXACT, None, pc.GRID_HYP, pc.GRID_SEED, 0, pc.GRID_TAU, None),
            ("grid_offset", pc.grid_cloud(), None, 65, 2 ** 63 + 11, 3 * pc.GRID_HYP, pc.GRID_TAU, None),
            ("table_normals", pts, nrm, 130, 1, 0, pc.TAU, float(np.cos(pc.NORMAL_ANGLE)))]


def _write(path, pts, nrm, n_hyp, seed, offset, tau, cos_theta):
    with open(path, "w") as f:
        f.write("%d %d %d %d %s %s\n" % (pts.shape[0], n_hyp, seed, offset, float(tau).hex(),
                                         float(-1.0 if cos_theta is None else cos_theta).hex()))
        for rows in ((pts,) if cos_theta is None else (pts, nrm)):
            for r in rows:
                f.write(" ".join(float(v).hex() for v in r) + "\n")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plane_seg") / "plane_seg_check")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fsanitize=float-cast-overflow",
           "-fno-sanitize-recover=undefined,float-cast-overflow", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "plane_seg_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout
    return exe


def test_header_decisions_equal_the_restatement_bit_for_bit(program, tmp_path):
    cases = _cases()
    paths = []
    for name, pts, nrm, n_hyp, seed, offset, tau, cos_theta in cases:
        paths.append(str(tmp_path / (name + ".txt")))
        _write(paths[-1], pts, nrm, n_hyp, seed, offset, tau, cos_theta)
    run = subprocess.run([program] + paths, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert run.returncode == 0, run.stdout[-4000:]
    lines = run.stdout.splitlines()
    assert lines[-1] == "plane_seg_check ok"
    at = 0
    for name, pts, nrm, n_hyp, seed, offset, tau, cos_theta in cases:
        assert lines[at] == "cloud %d %d" % (pts.shape[0], n_hyp), name
        b = op.build(pts, seed, n_hyp, offset)
        count, total, _ = op.score(pts, b["planes"], b["valid"], tau, nrm, cos_theta)
        rows = [ln.split() for ln in lines[at + 1:at + 1 + n_hyp]]
        assert all(r[0] == "hyp" and int(r[1]) == h for h, r in enumerate(rows)), name
        assert np.array_equal(np.array([[int(v) for v in r[2:5]] for r in rows]), b["triples"]), name
        assert np.array_equal(np.array([int(r[5]) for r in rows]) != 0, b["valid"]), name
        planes = np.array([[float.fromhex(v) for v in r[6:12]] for r in rows])
        assert np.array_equal(_bits(planes), _bits(b["planes"])), name
        assert np.array_equal(np.array([int(r[12]) for r in rows]), count), name
        assert np.array_equal(_bits([float.fromhex(r[13]) for r in rows]), _bits(total)), name
        w = op.winner(count, total)
        assert lines[at + 1 + n_hyp] == "winner %d" % w, name
        at += 2 + n_hyp
        if w < 0:
            continue
        inl, _ = op.inliers(pts, b["planes"][w], tau, nrm, cos_theta)
        t = op.refit_sums(pts, b["planes"][w], inl[0])
        got = lines[at].split()
        assert got[0] == "sums" and np.array_equal(_bits([float.fromhex(v) for v in got[1:]]), _bits(t)), name
        at += 1
        if t[0] >= 3.0:
            c, m = op.covariance(t)
            got = lines[at].split()
            want = np.concatenate([c, [m[0, 0], m[0, 1], m[0, 2], m[1, 1], m[1, 2], m[2, 2]]])
            assert got[0] == "cov" and np.array_equal(_bits([float.fromhex(v) for v in got[1:]]), _bits(want)), name
            at += 1
    assert at == len(lines) - 1


def test_interface_and_argument_checks_need_no_gpu(monkeypatch):
    import inspect

    from probreg_amd import dist, preprocess as pp

    assert pp.PlaneSegmentation._fields == ("plane", "point", "inliers", "mask", "distance", "fitness", "inlier_rmse",
                                            "hypothesis", "n_valid", "count", "sum")
    assert pp.PlaneSet._fields == ("planes", "points", "labels", "sizes", "n_planes")
    sig = inspect.signature(pp.segment_plane)
    assert list(sig.parameters)[:8] == ["points", "distance_threshold", "num_iterations", "seed", "refine_iters", "normals",
                                        "max_normal_angle", "device"]
    assert [sig.parameters[k].default for k in ("num_iterations", "seed", "refine_iters")] == [1000, 0, 3]
    sig = inspect.signature(pp.segment_planes)
    assert list(sig.parameters) == ["points", "distance_threshold", "max_planes", "min_inliers", "num_iterations", "seed",
                                    "refine_iters", "normals", "max_normal_angle", "device"]
    assert sig.parameters["min_inliers"].default == 3
    ok = np.random.default_rng(0).normal(size=(10, 3))
    nan = ok.copy()
    nan[3, 1] = np.nan
    bad = [dict(points=ok[:2]), dict(points=ok[:, :2]), dict(points=np.zeros((4, 3, 3))), dict(points=nan),
           dict(distance_threshold=-0.1), dict(distance_threshold=np.nan), dict(distance_threshold=np.inf),
           dict(num_iterations=0), dict(num_iterations=2.5), dict(refine_iters=-1), dict(max_normal_angle=0.3),
           dict(normals=ok[:5], max_normal_angle=0.3), dict(normals=ok, max_normal_angle=-0.1),
           dict(normals=ok, max_normal_angle=np.nan)]
    for kw in bad:
        args = dict(points=ok, distance_threshold=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            pp.segment_plane(**args)
        with pytest.raises(ValueError):
            pp.segment_planes(max_planes=2, **args)
    with pytest.raises(ValueError):
        pp.segment_planes(ok, 0.1, -1)
    with pytest.raises(ValueError):
        pp.segment_planes(ok, 0.1, 2, min_inliers=-1)
    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        pp.segment_plane(ok, 0.1)
    with pytest.raises(NotImplementedError):
        pp.segment_planes(ok, 0.1, 2)


def test_abi_argument_checks_need_no_gpu():
    import ctypes

    from probreg_amd import _lib

    lib = _lib.lib
    a = np.zeros((4, 6))
    pa = _lib.ptr(a)
    n64, cnt, sm = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_double(0.0)
    for fn, args in ((lib.prg_plane_create, (None, 0, None)), (lib.prg_plane_set_points, (None, pa, None, 4)),
                     (lib.prg_plane_count, (None, ctypes.byref(n64))), (lib.prg_plane_build, (None, 0, 0, 16)),
                     (lib.prg_plane_get_hypotheses, (None, None, None, None)), (lib.prg_plane_set_hypotheses, (None, pa, pa, 4)),
                     (lib.prg_plane_score, (None, 0.1, -1.0)), (lib.prg_plane_get_scores, (None, None, None)),
                     (lib.prg_plane_best, (None, ctypes.byref(n64), ctypes.byref(n64), ctypes.byref(cnt), ctypes.byref(sm), None)),
                     (lib.prg_plane_refine, (None, 0.1, -1.0, 3, pa, None)),
                     (lib.prg_plane_classify, (None, pa, 0.1, -1.0, None, None, ctypes.byref(cnt), ctypes.byref(sm))),
                     (lib.prg_plane_remove, (None, ctypes.byref(n64)))):
        assert fn(*args) == _lib.PRG_ERR_INVALID
        assert "NULL" in _lib.last_error()
    assert lib.prg_plane_destroy(None) == _lib.PRG_OK


def test_no_gpu_fails_loudly():
    """Without a GPU the entry points raise instead of computing on the CPU."""
    from probreg_amd import _lib, preprocess as pp

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    x = pc.lattices()
    with pytest.raises(_lib.ProbregHipError):
        pp.PlanePlan()
    with pytest.raises(_lib.ProbregHipError):
        pp.segment_plane(x, 0.1)
    with pytest.raises(_lib.ProbregHipError):
        pp.segment_planes(x, 0.1, 2)
