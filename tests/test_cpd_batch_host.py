"""registration_cpd_batch without a GPU: argument errors are raised before the device is touched, the sweep's tile table covers
every column of every problem exactly once and a problem's tiles depend on its own sizes only, one (B, M, D) array is the same
input as a list of clouds, and a valid call on a machine without a GPU fails loudly."""
import numpy as np
import pytest

from probreg_amd import _lib, cpd, engine


def _clouds(b, m, n, dim=3, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=(m, dim)) for _ in range(b)], [rng.normal(size=(n, dim)) for _ in range(b)]


def test_argument_errors_are_value_errors(monkeypatch):
    def no_gpu_call():
        raise AssertionError("the GPU was touched before the arguments were checked")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu_call)
    src, tgt = _clouds(3, 20, 25)
    bad = [
        dict(sources=src, targets=tgt[:2]),                                   # length mismatch
        dict(sources=[], targets=[]),                                         # nothing to do
        dict(sources=src, targets=tgt, tf_type_name="nonrigid"),              # a kind that is not batched
        dict(sources=src, targets=tgt, tf_type_name="similarity"),            # an unknown kind
        dict(sources=[src[0], src[1][:, :2], src[2]], targets=tgt),           # mixed D inside the sources
        dict(sources=[s[:, :2] for s in src], targets=tgt),                   # sources 2-D, targets 3-D
        dict(sources=[src[0], np.zeros((0, 3)), src[2]], targets=tgt),        # an empty source
        dict(sources=src, targets=[tgt[0], tgt[1], np.zeros((0, 3))]),        # an empty target
        dict(sources=[np.zeros((5, 4))] * 3, targets=[np.zeros((5, 4))] * 3),  # D = 4
        dict(sources=np.zeros((3, 20)), targets=tgt),                         # one array that is not (B, M, D)
        dict(sources=src, targets=tgt, w=[0.1, 0.2]),                         # w: neither a scalar nor one per problem
        dict(sources=src, targets=tgt, tol=np.zeros(4)),                      # tol likewise
        dict(sources=src, targets=tgt, w=1.0),                                # w outside [0, 1)
        dict(sources=src, targets=tgt, tf_init_params=[{}, {}]),              # init dicts: wrong count
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            cpd.registration_cpd_batch(**kw)


def test_array_input_is_the_same_batch_as_list_input():
    src, tgt = _clouds(4, 17, 23, seed=3)
    a = cpd._batch_clouds(np.stack(src), "sources")
    b = cpd._batch_clouds(src, "sources")
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.dtype == np.float64 and x.shape == (17, 3) and np.array_equal(x, y)
    f32 = cpd._batch_clouds(np.stack(tgt).astype(np.float32), "targets")
    assert all(c.dtype == np.float64 for c in f32)


def _check_table(ms, ns):
    tile_cols, _chunk = engine.batch_tile_shape()
    table = engine.batch_tile_table(ms, ns)
    assert table.dtype == np.int32 and table.shape[1] == 3
    # launch order: problem by problem, columns ascending
    assert np.all(np.diff(table[:, 0]) >= 0)
    for b, n in enumerate(ns):
        mine = table[table[:, 0] == b]
        assert len(mine) == -(-n // tile_cols)
        seen = np.zeros(n, dtype=np.int64)
        for _, first, count in mine:
            assert 0 <= first and 1 <= count <= tile_cols and first + count <= n   # stays within its problem
            seen[first:first + count] += 1
        assert np.all(seen == 1)                                                    # every column exactly once
    return table


def test_tile_table_covers_every_column_once_and_is_per_problem():
    tile_cols, chunk = engine.batch_tile_shape()
    assert tile_cols >= 64 and chunk >= 4
    ms = [5, 33, 64, 255, 300, 1000, 513, chunk - 1, chunk, chunk + 1]
    ns = [7, 31, 257, 256, 1000, 300, 129, tile_cols - 1, tile_cols, tile_cols + 1]
    table = _check_table(ms, ns)
    # a problem's tiles do not change when other problems are added, in front of it or behind it
    for b in range(len(ms)):
        alone = engine.batch_tile_table([ms[b]], [ns[b]])
        assert np.array_equal(alone[:, 1:], table[table[:, 0] == b][:, 1:])
    rev = _check_table(ms[::-1], ns[::-1])
    for b in range(len(ms)):
        assert np.array_equal(rev[rev[:, 0] == len(ms) - 1 - b][:, 1:], table[table[:, 0] == b][:, 1:])
    # ... nor with the source's size (the tile rule is a function of N_b; M_b sets the trip count of the tile's loop)
    assert np.array_equal(engine.batch_tile_table([7], [1000])[:, 1:], engine.batch_tile_table([4000], [1000])[:, 1:])


def test_tile_table_rejects_empty_problems():
    with pytest.raises(ValueError):
        engine.batch_tile_table([10, 0], [10, 10])
    with pytest.raises(ValueError):
        engine.batch_tile_table([10, 10], [10])


def test_valid_call_without_a_gpu_fails_loudly():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    src, tgt = _clouds(2, 20, 25)
    with pytest.raises(_lib.ProbregHipError):
        cpd.registration_cpd_batch(src, tgt)
