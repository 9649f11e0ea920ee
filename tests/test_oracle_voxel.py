"""The restatement of voxel down-sampling (tests/oracle_voxel.py) against a direct computation, and
the conditions under which the GPU tests may compare with it exactly.  No GPU."""
import math

import numpy as np
import pytest

import oracle_voxel as ov


def _direct(points, v, channel=None):
    """A dictionary of cells filled in input order, with math.fsum means: no sort, no pieces, no ordered sums."""
    lo = points.min(axis=0) - 0.5 * v
    members = {}
    for i, p in enumerate(points):
        members.setdefault(tuple(int(math.floor((p[a] - lo[a]) / v)) for a in range(points.shape[1])), []).append(i)
    cells = sorted(members)  # tuples compare lexicographically: (c_x, c_y[, c_z]) ascending
    values = points if channel is None else channel
    means = np.array([[math.fsum(values[members[c], k]) / len(members[c]) for k in range(values.shape[1])] for c in cells])
    inverse = np.empty(points.shape[0], dtype=np.int64)
    for r, c in enumerate(cells):
        inverse[members[c]] = r
    return (np.array(cells), means, np.array([len(members[c]) for c in cells]), np.array([members[c][0] for c in cells]),
            inverse)


def _cases():
    yield "across 0.1", ov.across_case(), ov.ACROSS_V[0]
    yield "across 0.03", ov.across_case(), ov.ACROSS_V[1]
    yield ("faces",) + ov.faces_case()[:2]
    yield ("planar",) + ov.planar_case()
    yield ("one voxel 1000",) + ov.one_voxel_case(1000)
    yield ("alone",) + ov.alone_case()
    yield ("channels",) + ov.channel_case()[::2]
    for name in ("one", "pair_together", "pair_apart"):
        yield (name,) + ov.edge_case(name)


@pytest.mark.parametrize("name,points,v", list(_cases()), ids=[c[0] for c in _cases()])
def test_restatement_equals_a_direct_computation(name, points, v):
    ref = ov.down_sample(points, v)
    cells, means, counts, first, inverse = _direct(points, v)
    d = points.shape[1]
    assert np.array_equal(np.unique(ref["cells"], axis=0)[:, :d], cells)
    assert np.array_equal(ref["cells"][ref["first"]][:, :d], cells)  # the rows come in ascending (c_x, c_y, c_z)
    assert np.array_equal(ref["counts"], counts) and ref["counts"].dtype == np.int32
    assert np.array_equal(ref["first"], first) and np.array_equal(ref["inverse"], inverse)
    bound = counts[:, None] * 2.0 ** -52 * np.max(np.abs(points))
    err = np.abs(ref["points"] - means)
    print("%s: V = %d, largest count = %d, mean err / bound = %.3f" % (name, len(counts), counts.max(), np.max(err / bound)))
    assert np.all(err <= bound)


def test_restatement_of_the_channels_equals_a_direct_computation():
    points, normals, v = ov.channel_case()
    attributes = ov.attribute_case(7)
    ref = ov.down_sample(points, v, normals=normals, attributes=attributes)
    for name, channel in (("normals", normals), ("attributes", attributes)):
        _, means, counts, _, _ = _direct(points, v, channel)
        assert np.all(np.abs(ref[name] - means) <= counts[:, None] * 2.0 ** -52 * np.max(np.abs(channel)))
    # the far voxel: its two normals cancel, the mean is 0 and stays 0 under unit_normals; every other row becomes a unit vector
    unit = ov.down_sample(points, v, normals=normals, unit_normals=True)["normals"]
    assert ref["counts"][-1] == 2 and np.all(ref["normals"][-1] == 0.0) and np.all(unit[-1] == 0.0)
    assert np.all(np.abs(np.linalg.norm(unit[:-1], axis=1) - 1.0) < 1.0e-15 * 4)


def test_order_inside_a_voxel_and_the_pieces():
    points = ov.across_case()
    ref = ov.down_sample(points, ov.ACROSS_V[0])
    o, rows = ref["order"], ref["rows"]
    same = rows[1:] == rows[:-1]
    assert np.all(o[1:][same] > o[:-1][same])  # ascending original index inside a run
    assert np.array_equal(np.sort(o), np.arange(points.shape[0]))
    pieces = ov.piece_sums(points[o], rows)
    assert all(a[0] < b[0] or (a[0] == b[0] and a[1] < b[1]) for a, b in zip(pieces, pieces[1:]))
    assert len(pieces) > len(ref["counts"])  # some voxel has more than one piece
    # one voxel of 129 points: pieces of 64, 64 and 1, and the two-level sum is those three added in order
    pts, v = ov.one_voxel_case(129)
    ref = ov.down_sample(pts, v)
    parts = [pts[:64], pts[64:128], pts[128:]]
    total = np.zeros(3)
    for part in parts:
        acc = np.zeros(3)
        for row in part:
            acc = acc + row
        total = total + acc
    assert np.array_equal(ref["order"], np.arange(129)) and np.array_equal(ref["points"][0], total / 129.0)


def _gpu_cases():
    """Every (points, v) the GPU tests compare exactly, except the case built to sit on faces."""
    out = list(_cases())
    out += [("one voxel %d" % n,) + ov.one_voxel_case(n) for n in ov.ONE_VOXEL_N]
    out += [("width %s" % k,) + ov.width_case(k) for k in "ABCD"]
    out += [("reuse %d" % i, ov._surface(n, seed), v) for i, (n, seed, v) in enumerate(ov.REUSE)]
    return [c for c in out if c[0] != "faces"]


def test_every_gpu_case_is_safe():
    """No quotient (p - lo) / v lies within BAND (relative) of an integer, so an fp64 implementation that rounds every
    operation once cannot put a point into another cell; where points do sit on faces, the arithmetic is exact."""
    for name, points, v in _gpu_cases():
        margin = ov.down_sample(points, v)["margin"]
        assert margin > ov.BAND, (name, margin)
    points, v, m = ov.faces_case()
    ref = ov.down_sample(points, v)
    assert ref["margin"] == 0.0  # on faces
    lo = points.min(axis=0) - 0.5 * v
    assert np.array_equal(lo, [-0.125] * 3)
    assert np.array_equal((points - lo) / v * 2.0, (m + 1).astype(np.float64))  # the quotients are exact
    assert np.array_equal(ref["cells"], (m + 1) // 2)
    assert np.any((m + 1) % 2 == 0) and ref["counts"].max() >= 50


def test_every_point_alone_and_all_points_together():
    points, v = ov.alone_case()
    ref = ov.down_sample(points, v)
    assert ref["counts"].shape[0] == points.shape[0] and np.all(ref["counts"] == 1)
    assert np.array_equal(ref["points"], points[ref["order"]])  # (0.0 + p) / 1.0 == p
    for n in ov.ONE_VOXEL_N:
        points, v = ov.one_voxel_case(n)
        assert np.array_equal(ov.down_sample(points, v)["counts"], [n])
    for v_across in ov.ACROSS_V:
        ref = ov.down_sample(ov.across_case(), v_across)
        assert ref["counts"].shape[0] > 64 and ov.crosses_a_block(ref["rows"])


def test_index_range():
    for name, axis in (("A", 0), ("B", 1), ("C", 2), ("D", 0)):
        points, v = ov.width_case(name)
        ref = ov.down_sample(points, v)
        assert ref["cells"].max() == ov.MAX_CELLS - 1 and np.array_equal(ref["counts"], [1, 1])
        with pytest.raises(ValueError, match="axis %d" % axis):
            ov.down_sample(*ov.width_case(name, ov.WIDTH + 1.0))
    assert int(ov.down_sample(*ov.width_case("D"))["keys"][1]) == 2 ** 63 - 1


def test_end_to_end_case_stays_within_half_of_its_bound():
    """oracle_voxel, then oracle_fpfh, then oracle_global_reg on the family-F clouds at n = 20000: the pose lies within half of
    (6 degrees, 0.05), the bound of test_voxel_gpu.test_pose_of_registration_global_with_voxel_size.
    Measured: 2426 and 2600 voxels, 588 mutual matches, rot_err = 0.707 degrees, t_err = 0.0089."""
    ref = ov.e2e_restatement()
    for cloud in (ref["source"], ref["target"]):
        assert ov.E2E_VOXELS[0] <= cloud.shape[0] <= ov.E2E_VOXELS[1]
    assert ref["margin"] > ov.BAND and ref["ransac"]["band"] == 0
    rot_err, t_err = ref["error"]
    print("voxels: %d, %d; matches: %d; rot_err = %.4f deg, t_err = %.5f"
          % (ref["source"].shape[0], ref["target"].shape[0], ref["pairs"].shape[0], rot_err, t_err))
    assert rot_err < 3.0 and t_err < 0.025
