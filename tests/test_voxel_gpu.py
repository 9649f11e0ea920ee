"""Voxel down-sampling on the GPU (probreg_amd.preprocess, csrc/voxel.hip) against its restatement (tests/oracle_voxel.py,
DESIGN.md section 3.14), stage by stage and through the public call.

Everything is compared to the last bit - keys, order, rows, counts, first, inverse and the means: the CPU tests
(test_oracle_voxel.py) show that no cell decision of these cases lies within 1e-9 (relative) of a face of the grid unless the
arithmetic of the case is exact, and the definition fixes the order of every sum.
"""
import functools
import math

import numpy as np
import pytest

import oracle_voxel as ov
from probreg_amd import preprocess

pytestmark = pytest.mark.gpu

STAGES = ("keys", "order", "rows", "points", "counts", "first", "inverse")


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _stages(plan, channels=False):
    out = {"keys": plan.keys(), "order": plan.order(), "rows": plan.rows(), "points": plan.means(), "counts": plan.counts(),
           "first": plan.first(), "inverse": plan.inverse(), "V": plan.count()}
    if channels:
        out["channels"] = plan.channel_means()
    return out


def _run(points, v, channels=None):
    plan = preprocess.VoxelPlan()
    try:
        plan.set_data(points)
        if channels is not None:
            plan.set_channels(channels)
        plan.run(v)
        return _stages(plan, channels is not None)
    finally:
        plan.close()


def _check(got, ref):
    assert got["V"] == ref["counts"].shape[0]
    for name in STAGES:
        assert _same(got[name], ref[name]), name


# ------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("name,counts", [("one", [1]), ("pair_together", [2]), ("pair_apart", [1, 1])])
def test_edges_of_n(name, counts):
    points, v = ov.edge_case(name)
    got = _run(points, v)
    _check(got, ov.down_sample(points, v))
    assert np.array_equal(got["counts"], counts)
    res = preprocess.voxel_down_sample(points, v)
    assert _same(res.points, got["points"]) and res.normals is None and res.attributes is None
    assert _same(res.counts, got["counts"]) and _same(res.first, got["first"]) and _same(res.inverse, got["inverse"])


@pytest.mark.parametrize("n", ov.ONE_VOXEL_N)
def test_piece_boundaries_with_all_points_in_one_voxel(n):
    points, v = ov.one_voxel_case(n)
    got = _run(points, v)
    _check(got, ov.down_sample(points, v))
    assert got["points"].shape == (1, 3) and np.array_equal(got["counts"], [n])
    assert np.array_equal(got["order"], np.arange(n)) and np.all(got["inverse"] == 0) and got["first"][0] == 0


def test_every_point_alone():
    points, v = ov.alone_case()
    ref = ov.down_sample(points, v)
    n = points.shape[0]
    assert ref["counts"].shape[0] == n
    got = _run(points, v)
    _check(got, ref)
    assert _same(got["points"], np.ascontiguousarray(points[got["order"]]))  # the inputs bit for bit, in key order
    assert np.array_equal(got["first"], got["order"])
    assert np.array_equal(got["inverse"][got["order"]], np.arange(n)) and np.array_equal(got["rows"], np.arange(n))


@pytest.mark.parametrize("v", ov.ACROSS_V)
def test_runs_across_blocks(v):
    points = ov.across_case()
    ref = ov.down_sample(points, v)
    assert ref["counts"].shape[0] > 64 and ov.crosses_a_block(ref["rows"])
    _check(_run(points, v), ref)


def test_points_on_faces_in_exact_arithmetic():
    points, v, m = ov.faces_case()
    got = _run(points, v)
    cells = (m + 1) // 2  # integer arithmetic
    keys = (cells[:, 0].astype(np.uint64) << np.uint64(42)) | (cells[:, 1].astype(np.uint64) << np.uint64(21)) \
        | cells[:, 2].astype(np.uint64)
    assert _same(got["keys"], keys)
    _check(got, ov.down_sample(points, v))
    assert np.any(np.signbit(points)) and got["counts"].max() >= 50
    dup = got["inverse"][99]
    assert np.all(got["inverse"][100:150] == dup) and got["first"][dup] <= 99


# --------------------------------------------------------------------------------------------------------- key width
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_key_width(name):
    points, v = ov.width_case(name)
    ref = ov.down_sample(points, v)
    assert ref["cells"].max() == ov.MAX_CELLS - 1
    got = _run(points, v)
    _check(got, ref)
    assert np.array_equal(got["order"], [0, 1]) and _same(got["points"], np.ascontiguousarray(points))


@pytest.mark.parametrize("name,axis", [("A", 0), ("B", 1), ("C", 2)])
def test_index_range_overflow_names_the_axis_and_leaves_the_plan_usable(name, axis):
    from probreg_amd import _lib

    points, v = ov.width_case(name, ov.WIDTH + 1.0)
    plan = preprocess.VoxelPlan()
    try:
        plan.set_data(points)
        with pytest.raises(ValueError, match=r"axis %d .*2\.09715e\+06.*voxel_size 1 " % axis):
            plan.run(v)
        with pytest.raises(_lib.ProbregHipError):  # nothing was sorted: there is no result
            plan.means()
        plan.run(2.0 * v)  # the same cloud on a coarser grid
        _check(_stages(plan), ov.down_sample(points, 2.0 * v))
        good, v_good = ov.width_case(name)
        plan.set_data(good)
        plan.run(v_good)
        _check(_stages(plan), ov.down_sample(good, v_good))
    finally:
        plan.close()
    with pytest.raises(ValueError, match="axis %d" % axis):
        preprocess.voxel_down_sample(points, v)


# --------------------------------------------------------------------------------------------------- d = 2, channels
def test_planar_cloud():
    points, v = ov.planar_case()
    normals = np.random.default_rng(32).normal(size=points.shape)
    ref = ov.down_sample(points, v, normals=normals)
    assert np.all(ref["cells"][:, 2] == 0)
    _check(_run(points, v), ref)
    res = preprocess.voxel_down_sample(points, v, normals=normals)
    assert res.points.shape[1] == 2 and _same(res.points, ref["points"]) and _same(res.normals, ref["normals"])


def test_normals_alone_and_unit_normals():
    points, normals, v = ov.channel_case()
    ref = ov.down_sample(points, v, normals=normals)
    res = preprocess.voxel_down_sample(points, v, normals=normals)
    assert _same(res.points, ref["points"]) and _same(res.normals, ref["normals"]) and res.attributes is None
    assert _same(res.counts, ref["counts"]) and _same(res.first, ref["first"]) and _same(res.inverse, ref["inverse"])
    assert np.all(np.linalg.norm(res.normals, axis=1) <= 1.0 + 1.0e-15)  # means of unit vectors, not renormalised
    unit = preprocess.voxel_down_sample(points, v, normals=normals, unit_normals=True)
    norm = np.sqrt(res.normals[:, 0] * res.normals[:, 0] + res.normals[:, 1] * res.normals[:, 1]
                   + res.normals[:, 2] * res.normals[:, 2])
    assert res.counts[-1] == 2 and norm[-1] == 0.0 and np.count_nonzero(norm == 0.0) == 1  # the normals that cancel
    assert _same(unit.normals[:-1], res.normals[:-1] / norm[:-1, None]) and np.all(unit.normals[-1] == 0.0)
    assert _same(unit.normals, ov.down_sample(points, v, normals=normals, unit_normals=True)["normals"])
    assert _same(unit.points, res.points)

    class Cloud(object):  # an object's normals are used when none are given
        pass

    cloud = Cloud()
    cloud.points, cloud.normals = points, normals
    assert _same(preprocess.voxel_down_sample(cloud, v).normals, res.normals)
    cloud.normals = normals[:5]  # not one per point: ignored
    assert preprocess.voxel_down_sample(cloud, v).normals is None


@pytest.mark.parametrize("c", ov.CHANNEL_C)
def test_attributes(c):
    points, normals, v = ov.channel_case()
    attributes = ov.attribute_case(c)
    ref = ov.down_sample(points, v, normals=normals, attributes=attributes)
    res = preprocess.voxel_down_sample(points, v, attributes=attributes)
    assert res.normals is None and res.attributes.shape == (ref["counts"].shape[0], c)
    assert _same(res.attributes, ref["attributes"]) and _same(res.points, ref["points"])
    both = preprocess.voxel_down_sample(points, v, normals=normals, attributes=attributes)
    assert _same(both.attributes, ref["attributes"]) and _same(both.normals, ref["normals"])
    assert _same(both.points, ref["points"]) and _same(both.inverse, ref["inverse"])


# -------------------------------------------------------------------------------------------------------- invariants
def test_invariants_and_a_permuted_input():
    points = ov.across_case()
    v = ov.ACROSS_V[0]
    n = points.shape[0]
    res = preprocess.voxel_down_sample(points, v)
    cells = ov.cells(points, v)[0]
    assert res.counts.sum() == n and res.counts.min() >= 1
    assert np.array_equal(cells[res.first[res.inverse]], cells)  # every point lies in the cell of its voxel
    assert np.array_equal(np.bincount(res.inverse, minlength=res.counts.shape[0]), res.counts)
    lo = points.min(axis=0) - 0.5 * v
    slack = 4.0 * np.finfo(np.float64).eps * np.max(np.abs(points))
    box = lo + cells[res.first] * v
    assert np.all(res.points >= box - slack) and np.all(res.points <= box + v + slack)  # so does the mean
    for a in range(3):
        total = math.fsum(res.counts * res.points[:, a])
        assert abs(total - math.fsum(points[:, a])) <= n * 2.0 ** -52 * math.fsum(np.abs(points[:, a]))
    perm = np.random.default_rng(5).permutation(n)
    shuffled = preprocess.voxel_down_sample(np.ascontiguousarray(points[perm]), v)
    assert np.array_equal(shuffled.counts, res.counts)
    assert np.array_equal(cells[perm][shuffled.first], cells[res.first])
    assert np.array_equal(shuffled.inverse, res.inverse[perm])
    assert np.all(np.abs(shuffled.points - res.points) <= res.counts[:, None] * 2.0 ** -52 * np.max(np.abs(points)))


def test_two_runs_are_byte_identical():
    points, normals, v = ov.channel_case()
    attributes = ov.attribute_case(7)
    a = preprocess.voxel_down_sample(points, v, normals=normals, attributes=attributes)
    b = preprocess.voxel_down_sample(points, v, normals=normals, attributes=attributes)
    for x, y in zip(a, b):
        assert _same(x, y)


def test_plan_reuse():
    """One plan at n = 5000, then n = 70 (with channels), then n = 5000 with another v (without): each run equals a fresh plan's
    and the restatement's."""
    plan = preprocess.VoxelPlan()
    try:
        for i, (n, seed, v) in enumerate(ov.REUSE):
            points = ov._surface(n, seed)
            channels = np.random.default_rng(seed).normal(size=(n, 5)) if i == 1 else None
            plan.set_data(points)
            if channels is not None:
                plan.set_channels(channels)
            plan.run(v)
            got = _stages(plan, channels is not None)
            fresh = _run(points, v, channels)
            ref = ov.down_sample(points, v, attributes=channels)
            _check(got, ref)
            for name in STAGES:
                assert _same(got[name], fresh[name]), name
            if channels is not None:
                assert _same(got["channels"], ref["attributes"]) and _same(fresh["channels"], ref["attributes"])
            else:
                assert plan.n_channels == 0
    finally:
        plan.close()


def test_abi_argument_errors_on_a_handle():
    from probreg_amd import _lib

    lib = _lib.lib
    points = ov._surface(70, 12)
    out = np.zeros(70 * 3)
    plan = preprocess.VoxelPlan()
    try:
        h = plan._h
        assert lib.prg_voxel_run(h, 0.1) == _lib.PRG_ERR_STATE
        assert lib.prg_voxel_set_channels(h, _lib.ptr(points), 3) == _lib.PRG_ERR_STATE
        assert lib.prg_voxel_set_data(h, None, 70, 3) == _lib.PRG_ERR_INVALID
        for d in (1, 4):
            assert lib.prg_voxel_set_data(h, _lib.ptr(points), 70, d) == _lib.PRG_ERR_INVALID
        plan.set_data(points)
        for fn in (lib.prg_voxel_get_means, lib.prg_voxel_get_counts, lib.prg_voxel_get_first, lib.prg_voxel_get_inverse,
                   lib.prg_voxel_get_keys, lib.prg_voxel_get_order, lib.prg_voxel_get_rows, lib.prg_voxel_get_channel_means):
            assert fn(h, _lib.ptr(out)) == _lib.PRG_ERR_STATE, fn.__name__
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert lib.prg_voxel_run(h, v) == _lib.PRG_ERR_INVALID
        assert lib.prg_voxel_set_channels(h, None, 3) == _lib.PRG_ERR_INVALID
        assert lib.prg_voxel_set_channels(h, _lib.ptr(points), 68) == _lib.PRG_ERR_INVALID
        plan.run(0.2)
        assert lib.prg_voxel_get_means(h, None) == _lib.PRG_ERR_INVALID
        assert lib.prg_voxel_get_channel_means(h, _lib.ptr(out)) == _lib.PRG_ERR_STATE  # no channels were set
        _check(_stages(plan), ov.down_sample(points, 0.2))
    finally:
        plan.close()


# ------------------------------------------------------------------------------- composition with global registration
@functools.lru_cache(maxsize=None)
def _e2e():
    """(the composed call, the same by hand) on the family-F clouds at n = 20000."""
    import oracle_global_reg as og
    from probreg_amd import fpfh, global_reg

    src, tgt, _, _ = ov.e2e_clouds()
    kw = dict(feature_fn=fpfh.FPFH(*og.F_RADII), max_distance=og.F_TAU, n_hypotheses=og.F_HYP, seed=og.F_SEED)
    composed = global_reg.registration_global(src, tgt, voxel_size=ov.E2E_VOXEL, **kw)
    s = preprocess.voxel_down_sample(src, ov.E2E_VOXEL).points
    g = preprocess.voxel_down_sample(tgt, ov.E2E_VOXEL).points
    return composed, global_reg.registration_global(s, g, **kw), s, g


def _same_result(a, b):
    return (_same(a.transformation.rot, b.transformation.rot) and _same(a.transformation.t, b.transformation.t)
            and a.transformation.scale == b.transformation.scale and a.fitness == b.fitness
            and a.inlier_rmse == b.inlier_rmse and _same(a.inliers, b.inliers))


def test_registration_global_with_voxel_size_is_the_composition():
    import oracle_global_reg as og
    from probreg_amd import fpfh, global_reg

    composed, by_hand, s, g = _e2e()
    ref = ov.e2e_restatement()
    assert _same(s, ref["source"]) and _same(g, ref["target"])
    assert ov.E2E_VOXELS[0] <= s.shape[0] <= ov.E2E_VOXELS[1] and ov.E2E_VOXELS[0] <= g.shape[0] <= ov.E2E_VOXELS[1]
    assert _same_result(composed, by_hand)
    assert composed.inliers.max() < min(s.shape[0], g.shape[0])  # indices into the matches of the down-sampled clouds
    # without voxel_size: the stages as they were, on the clouds as they are
    src, tgt, _, _ = og.family_f_clouds(1)
    feature_fn = fpfh.FPFH(*og.F_RADII)
    kw = dict(n_hypotheses=og.F_HYP, seed=og.F_SEED)
    plain = global_reg.registration_global(src, tgt, feature_fn=feature_fn, max_distance=og.F_TAU, **kw)
    none = global_reg.registration_global(src, tgt, feature_fn=feature_fn, max_distance=og.F_TAU, voxel_size=None, **kw)
    pairs, _ = global_reg.feature_matching(feature_fn(src), feature_fn(tgt), True)
    stages = global_reg.registration_ransac(src, tgt, pairs, og.F_TAU, **kw)
    assert _same_result(plain, none) and _same_result(plain, stages)


def test_pose_of_registration_global_with_voxel_size():
    """The pose of the composed call against the ground truth of the full clouds: rot_err < 6 degrees and t_err < 0.05, the
    bound of test_end_to_end_family_f_and_a_local_method_started_from_it.  The restatement pipeline alone stays within half
    of it (test_oracle_voxel.test_end_to_end_case_stays_within_half_of_its_bound: 0.707 degrees, 0.0089).
    Measured on the GPU: 2426 and 2600 voxels, fitness 0.5119, rot_err = 0.707 degrees, t_err = 0.0089."""
    import oracle_global_reg as og

    composed = _e2e()[0]
    _, _, rot, t = ov.e2e_clouds()
    rot_err, t_err = og.pose_error(composed.transformation.rot, composed.transformation.t, rot, t)
    print("composed call: fitness = %.4f, rot_err = %.4f deg, t_err = %.5f" % (composed.fitness, rot_err, t_err))
    assert rot_err < 6.0 and t_err < 0.05
