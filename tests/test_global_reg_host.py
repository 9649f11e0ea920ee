"""Host-side behaviour of global registration (probreg_amd.global_reg): imports, argument checks, the no-GPU error.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest


def test_module_is_a_lazy_submodule():
    import probreg_amd

    assert "global_reg" in probreg_amd._SUBMODULES
    mod = probreg_amd.global_reg
    for name in ("feature_matching", "nearest_feature", "RansacPlan", "registration_ransac", "registration_global",
                 "GlobalResult"):
        assert hasattr(mod, name)
    assert mod.GlobalResult._fields == ("transformation", "fitness", "inlier_rmse", "inliers")
    assert "tf_init_params" in mod.__doc__


def test_signatures():
    from probreg_amd import global_reg as gr

    sig = inspect.signature(gr.registration_ransac)
    assert list(sig.parameters)[:8] == ["source", "target", "correspondences", "max_distance", "n_hypotheses",
                                        "edge_similarity", "refine_iters", "seed"]
    assert [sig.parameters[k].default for k in ("n_hypotheses", "edge_similarity", "refine_iters", "seed")] == [65536, 0.9, 3, 0]
    sig = inspect.signature(gr.registration_global)
    assert list(sig.parameters)[:5] == ["source", "target", "feature_fn", "max_distance", "mutual"]
    assert sig.parameters["feature_fn"].default is None and sig.parameters["mutual"].default is True
    assert inspect.signature(gr.feature_matching).parameters["mutual"].default is True


def test_feature_matching_rejects_bad_input_without_a_gpu():
    from probreg_amd import global_reg as gr

    ok = np.zeros((5, 33))
    nan = ok.copy()
    nan[1, 2] = np.nan
    for a, b in ((np.zeros(5), ok), (ok, np.zeros((4, 32))), (np.zeros((0, 33)), ok), (nan, ok), (ok, nan),
                 (np.zeros((5, 65)), np.zeros((5, 65))), (np.zeros((5, 0)), np.zeros((5, 0))), (np.zeros((2, 3, 4)), ok)):
        with pytest.raises(ValueError):
            gr.feature_matching(a, b)
        with pytest.raises(ValueError):
            gr.nearest_feature(a, b)
    with pytest.raises(ValueError, match="dimensions differ"):
        gr.feature_matching(ok, np.zeros((4, 32)))


def test_registration_ransac_rejects_bad_input_without_a_gpu():
    from probreg_amd import global_reg as gr

    src, tgt = np.zeros((10, 3)), np.ones((12, 3))
    corr = np.array([[0, 1], [1, 2], [2, 3], [3, 4]])
    inf = src.copy()
    inf[0, 0] = np.inf
    bad = [dict(source=np.zeros((10, 2))), dict(target=np.zeros(12)), dict(source=inf), dict(correspondences=corr[:2]),
           dict(correspondences=corr.astype(np.float64)), dict(correspondences=np.zeros((4, 3), dtype=np.int64)),
           dict(correspondences=np.array([[0, 1], [1, 2], [2, 12]])), dict(correspondences=np.array([[0, 1], [1, 2], [-1, 3]])),
           dict(correspondences=np.array([[10, 1], [1, 2], [2, 3]])), dict(max_distance=np.nan), dict(max_distance=np.inf),
           dict(max_distance=-0.1), dict(n_hypotheses=0), dict(n_hypotheses=2.5), dict(edge_similarity=1.5),
           dict(edge_similarity=np.nan), dict(refine_iters=-1)]
    for kw in bad:
        args = dict(source=src, target=tgt, correspondences=corr, max_distance=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            gr.registration_ransac(**args)
    with pytest.raises(ValueError, match="at least 3"):
        gr.registration_ransac(src, tgt, corr[:2], 0.1)


def test_registration_global_rejects_bad_input_without_a_gpu():
    from probreg_amd import global_reg as gr

    with pytest.raises(ValueError):
        gr.registration_global(np.zeros((10, 2)), np.zeros((10, 3)))
    with pytest.raises(ValueError):
        gr.registration_global(np.zeros((10, 3)), np.zeros((10, 3)), max_distance=np.nan)
    # descriptor dimensions that differ between the clouds
    with pytest.raises(ValueError, match="dimensions differ"):
        gr.registration_global(np.zeros((10, 3)), np.zeros((11, 3)), feature_fn=lambda x: np.zeros((x.shape[0], 3 + x.shape[0] % 2)))


def test_sharded_run_is_not_implemented(monkeypatch):
    from probreg_amd import dist, global_reg as gr

    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    x = np.random.default_rng(0).normal(size=(10, 3))
    with pytest.raises(NotImplementedError):
        gr.feature_matching(np.zeros((5, 33)), np.zeros((5, 33)))
    with pytest.raises(NotImplementedError):
        gr.registration_ransac(x, x, np.array([[0, 0], [1, 1], [2, 2]]), 0.1)
    with pytest.raises(NotImplementedError):
        gr.registration_global(x, x, feature_fn=lambda a: a)


def test_abi_argument_checks_need_no_gpu():
    from probreg_amd import _lib

    lib = _lib.lib
    a = np.zeros((4, 33))
    idx = np.zeros(4, dtype=np.int32)
    d2 = np.zeros(4)
    pa, pi, pd = _lib.ptr(a), _lib.ptr(idx), _lib.ptr(d2)
    assert lib.prg_feature_match(0, None, None, 4, pa, 4, 33, 0, pi, pd) == _lib.PRG_ERR_INVALID
    assert "NULL" in _lib.last_error()
    assert lib.prg_feature_match(0, None, pa, 4, pa, 4, 33, 0, None, pd) == _lib.PRG_ERR_INVALID
    for d in (0, 65, -1):
        assert lib.prg_feature_match(0, None, pa, 4, pa, 4, d, 0, pi, pd) == _lib.PRG_ERR_INVALID
        assert "1 .. 64" in _lib.last_error()
    assert lib.prg_feature_match(0, None, pa, 0, pa, 4, 33, 0, pi, pd) == _lib.PRG_ERR_INVALID
    assert lib.prg_feature_match(0, None, pa, 4, pa, 4, 33, -1, pi, pd) == _lib.PRG_ERR_INVALID
    assert lib.prg_feature_match_mutual(0, None, pa, 4, pa, 4, 33, 0, pi, pd, None) == _lib.PRG_ERR_INVALID
    assert "NULL" in _lib.last_error()
    cnt, sm, ind = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_int64(0)
    for fn, args in ((lib.prg_ransac_create, (None, 0, None)), (lib.prg_ransac_set_correspondences, (None, pa, pa, 4)),
                     (lib.prg_ransac_build, (None, 0, 0, 16, 0.9)), (lib.prg_ransac_get_hypotheses, (None, None, None, None)),
                     (lib.prg_ransac_set_hypotheses, (None, pa, pi, 4)), (lib.prg_ransac_score, (None, 0.1)),
                     (lib.prg_ransac_get_scores, (None, None, None)),
                     (lib.prg_ransac_best, (None, ctypes.byref(ind), ctypes.byref(cnt), ctypes.byref(sm), None)),
                     (lib.prg_ransac_refine, (None, 0.1, 3, None, ctypes.byref(cnt), ctypes.byref(sm), None))):
        assert fn(*args) == _lib.PRG_ERR_INVALID
        assert "NULL" in _lib.last_error()
    assert lib.prg_ransac_destroy(None) == _lib.PRG_OK


def test_no_gpu_fails_loudly():
    """Without a GPU every entry point raises instead of computing on the CPU."""
    from probreg_amd import _lib, global_reg as gr, synthetic

    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    x = synthetic.surface(40, 0)
    f = np.random.default_rng(0).uniform(size=(40, 33))
    with pytest.raises(_lib.ProbregHipError):
        gr.feature_matching(f, f)
    with pytest.raises(_lib.ProbregHipError):
        gr.RansacPlan()
    with pytest.raises(_lib.ProbregHipError):
        gr.registration_ransac(x, x, np.stack([np.arange(40), np.arange(40)], axis=1), 0.05)
    with pytest.raises(_lib.ProbregHipError):
        gr.registration_global(x, x + 0.1, max_distance=0.05)
