"""The shared cell grid (csrc/cell_grid.hip) through its two users, the FPFH search (csrc/fpfh.hip) and the ICP search (csrc/grid_search.hip), on the smallest
shapes at which the builder can go wrong: one bucket whose begin and end come from threads of two workgroups, a hashed grid
whose buckets hold several cells, and a single point.  Compared with the restatements as test_fpfh_gpu.py and
test_icp_gpu.py compare: FPFH indices and counts equal with d2 within 4 ulp, ICP (index, d2) byte for byte.
"""
import functools

import numpy as np
import pytest

import oracle_fpfh as ofp
import oracle_icp as oi
from probreg_amd import synthetic

pytestmark = pytest.mark.gpu

ULP4 = 4.0 * np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def _clouds():
    """X: 300 points of extent about 2.2; Y: X and one far point; Q: the 200 ICP queries."""
    x = ofp._f32(synthetic.surface(300, 5))
    y = ofp._f32(np.concatenate([x, [[900.0, -700.0, 800.0]]], axis=0))
    q = np.ascontiguousarray(synthetic.surface(200, 6) + 0.01)
    for v in (x, y, q):
        v.setflags(write=False)
    return x, y, q


def _fpfh_lists(points, radius, max_nn):
    from probreg_amd import fpfh
    plan = fpfh.FpfhPlan()
    try:
        plan.set_data(points)
        plan.search(fpfh.SEARCH_NORMALS, radius, max_nn)
        return plan.neighbours(fpfh.SEARCH_NORMALS)
    finally:
        plan.close()


def _check_lists(got, want):
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc)
    assert np.array_equal(gi, wi)
    assert np.all(np.abs(gd - wd) <= ULP4 * wd)


def _icp_matches(src, tgt, r, cell_edge):
    from probreg_amd import icp
    plan = icp.IcpPlan()
    try:
        plan.set_target(tgt, cell_edge=cell_edge)
        plan.set_source(src)
        plan.search(r)
        return plan.matches(), plan.grid()
    finally:
        plan.close()


def _same(got, ref):
    return got[0].dtype == np.int32 and got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


# ------------------------------------------------------------------------------------ one bucket across a block edge
@pytest.mark.parametrize("max_nn,count", [(512, 300), (30, 30)])
def test_fpfh_single_bucket_of_two_workgroups(max_nn, count):
    x, _, _ = _clouds()
    wi, wd, wc, fragile = ofp.hybrid_search(x, 10.0, max_nn)
    assert int(fragile.sum()) == 0 and np.all(wc == count)
    got = _fpfh_lists(x, 10.0, max_nn)
    assert np.all(got[2] == count)
    _check_lists(got, (wi, wd, wc))


@pytest.mark.parametrize("r", [0.05, np.inf])
def test_icp_single_bucket_of_two_workgroups(r):
    x, _, q = _clouds()
    got, (edge, dims, dense, levels) = _icp_matches(q, x, r, 10.0)
    assert edge == 10.0 and list(dims) == [1, 1, 1] and dense and levels == 1
    assert _same(got, oi.search(q, x, r))


# ------------------------------------------------------------------------------------------------------ hashed grid
def test_fpfh_hashed_grid():
    """About 4e12 cells of edge 0.05 against a table of 1024: keys are hashed, buckets hold several cells."""
    _, y, _ = _clouds()
    wi, wd, wc, fragile = ofp.hybrid_search(y, 0.05, 30)
    assert int(fragile.sum()) == 0 and wc.max() > 1 and wc[300] == 1
    _check_lists(_fpfh_lists(y, 0.05, 30), (wi, wd, wc))


@pytest.mark.parametrize("r,matched", [(0.05, 82), (np.inf, 200)])
def test_icp_hashed_grid(r, matched):
    _, y, q = _clouds()
    ref = oi.search(q, y, r)
    assert int((ref[0] >= 0).sum()) == matched
    got, (edge, dims, dense, _) = _icp_matches(q, y, r, 0.05)
    assert edge == 0.05 and not dense and float(np.prod(dims.astype(np.float64))) > 1.0e12
    assert int((got[0] >= 0).sum()) == matched
    assert _same(got, ref)


# ----------------------------------------------------------------------------------------------------- a single point
def test_one_point_is_first_and_last_of_its_bucket():
    x, _, q = _clouds()
    gi, gd, gc = _fpfh_lists(x[:1], 0.1, 30)
    assert gc.tolist() == [1] and gi[0, 0] == 0 and np.all(gi[0, 1:] == -1) and not gd.any()
    got, _ = _icp_matches(q, x[:1], np.inf, None)
    assert np.all(got[0] == 0) and _same(got, oi.search(q, x[:1], np.inf))
