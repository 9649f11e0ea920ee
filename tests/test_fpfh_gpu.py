"""The FPFH descriptor on the GPU (csrc/fpfh.hip through probreg_amd.fpfh), stage by stage against the restatement of
tests/oracle_fpfh.py.  The exact comparisons rest on test_oracle_fpfh.py: no point of clouds A, B, C is fragile.

Measured on one MI355X: the worst |n_gpu - n_ref| g / 1e-13 over A, B, C is 0.0042 (bound 1); SPFH and FPFH equal the
restatement's to the last bit, with the restatement's normals and with the device's own (bounds 1e-10 and 1e-9).

Cloud B with radius 10 (the whole cloud in range, cut to 100): the restatement reports 15 fragile points there, all from
"the last listed and the first cut d2 are closer than 1e-7 r^2".  That margin grows with r^2 = 100 while the spacing of
the 100 nearest d2 (about 4e-4) does not, so about 1 % of the points of any 1500-point cloud meet it and no seed gives
zero.  The comparison is made on every row all the same, the fragile ones included, and is exact.
"""
import numpy as np
import pytest

import oracle_fpfh as ofp

pytestmark = pytest.mark.gpu

ULP4 = 4.0 * np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def fp():
    from probreg_amd import fpfh
    return fpfh


def _plan(fp, points):
    plan = fp.FpfhPlan()
    plan.set_data(points)
    return plan


def _check_lists(got, want):
    gi, gd, gc = got
    wi, wd, wc = want
    assert np.array_equal(gc, wc)
    assert np.array_equal(gi, wi)
    assert np.all(np.abs(gd - wd) <= ULP4 * wd)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_both_searches_give_the_restatements_lists(fp, name):
    c = ofp.case(name)
    _, rn, rf = ofp.CASES[name]
    plan = _plan(fp, c["points"])
    plan.search(fp.SEARCH_NORMALS, rn, 30)
    plan.search(fp.SEARCH_FEATURES, rf, 100)
    _check_lists(plan.neighbours(fp.SEARCH_NORMALS), c["normal_lists"])
    _check_lists(plan.neighbours(fp.SEARCH_FEATURES), c["feature_lists"])
    plan.close()


def test_search_with_the_whole_cloud_in_range(fp):
    pts = ofp.cloud_b()
    wi, wd, wc, fragile = ofp.hybrid_search(pts, 10.0, 100)
    print("fragile points of cloud B at radius 10: %d" % int(fragile.sum()))
    assert np.all(wc == 100)
    plan = _plan(fp, pts)
    plan.search(fp.SEARCH_FEATURES, 10.0, 100)
    _check_lists(plan.neighbours(fp.SEARCH_FEATURES), (wi, wd, wc))
    plan.close()


def test_search_with_hashed_cell_keys(fp):
    """The 12 far points of cloud C at a small radius: the box has far more cells than the table, keys are hashed."""
    pts = ofp.cloud_c()
    wi, wd, wc, fragile = ofp.hybrid_search(pts, 0.05, 30)
    assert int(fragile.sum()) == 0
    plan = _plan(fp, pts)
    plan.search(fp.SEARCH_NORMALS, 0.05, 30)
    _check_lists(plan.neighbours(fp.SEARCH_NORMALS), (wi, wd, wc))
    plan.close()


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_normals_within_the_eigenvector_perturbation_bound(fp, name):
    """|n_gpu - n_ref| <= 1e-13 / g: first-order perturbation ||E|| / gap of the eigenvector, with ||E|| a few hundred
    eps lambda_max for 30 summands and a Jacobi solve.  Default normals are exact."""
    c = ofp.case(name)
    plan = _plan(fp, c["points"])
    plan.search(fp.SEARCH_NORMALS, ofp.CASES[name][1], 30)
    plan.compute_normals()
    got = plan.normals()
    plan.close()
    default = c["normal_lists"][2] < 3
    assert np.array_equal(got[default], np.tile([0.0, 0.0, 1.0], (int(default.sum()), 1)))
    err = np.max(np.abs(got - c["normals"]), axis=1)
    ratio = err[~default] * c["gap"][~default] / 1.0e-13
    print("cloud %s: worst |n_gpu - n_ref| g / 1e-13 = %.3g" % (name, ratio.max()))
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("own_normals", [False, True])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_histograms_no_rows_excluded(fp, name, own_normals):
    c = ofp.case(name)
    _, rn, rf = ofp.CASES[name]
    plan = _plan(fp, c["points"])
    if own_normals:
        plan.search(fp.SEARCH_NORMALS, rn, 30)
        plan.compute_normals()
    else:
        plan.set_normals(c["normals"])
    plan.search(fp.SEARCH_FEATURES, rf, 100)
    plan.compute_spfh()
    spfh = plan.spfh()
    plan.compute_fpfh()
    fpfh = plan.fpfh()
    plan.close()
    es, ef = np.max(np.abs(spfh - c["spfh"])), np.max(np.abs(fpfh - c["fpfh"]))
    print("cloud %s (%s normals): SPFH %.3g, FPFH %.3g" % (name, "device" if own_normals else "restatement", es, ef))
    assert fpfh.shape == (c["points"].shape[0], 33) and fpfh.dtype == np.float64
    assert es <= 1.0e-10
    assert ef <= 1.0e-9


def test_planar_cloud_gives_the_closed_form(fp):
    pts = ofp.cloud_p()
    _, rn, rf = ofp.CASES["P"]
    plan = _plan(fp, pts)
    plan.search(fp.SEARCH_NORMALS, rn, 30)
    assert plan.neighbours(fp.SEARCH_NORMALS)[2].min() >= 3
    plan.compute_normals()
    plan.search(fp.SEARCH_FEATURES, rf, 100)
    plan.compute_spfh()
    plan.compute_fpfh()
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(plan.normals(), np.tile([0.0, 0.0, 1.0], (500, 1)))
    assert np.array_equal(plan.spfh(), np.tile(want, (500, 1)))
    assert np.array_equal(plan.fpfh(), np.tile(2.0 * want, (500, 1)))
    plan.close()
    f = fp.FPFH(rn, rf)
    assert np.array_equal(f.compute(pts), np.tile(2.0 * want, (500, 1)))
    assert np.array_equal(f.normals_, np.tile([0.0, 0.0, 1.0], (500, 1)))


def test_compute_is_repeatable_and_handles_one_and_two_points(fp):
    pts = ofp.cloud_a()
    f = fp.FPFH()
    a = f.compute(pts)
    na = f.normals_.copy()
    b = f.compute(pts)
    assert a.tobytes() == b.tobytes() and na.tobytes() == f.normals_.tobytes()
    assert np.max(np.abs(a - ofp.case("A")["fpfh"])) <= 1.0e-9
    one = f.compute(pts[:1])
    assert one.shape == (1, 33) and not one.any()
    two = fp.FPFH(0.1, 10.0).compute(pts[:2])  # both default normals; each the other's only neighbour
    assert two.shape == (2, 33)
    for g in range(3):
        assert two[0, 11 * g:11 * g + 11].sum() == 200.0 and two[1, 11 * g:11 * g + 11].sum() == 200.0
    assert np.array_equal(two, ofp.describe(pts[:2], 0.1, 10.0)["fpfh"])
    far = fp.FPFH(0.1, 1.0e-3).compute(pts[:2])
    assert far.shape == (2, 33) and not far.any()


def test_estimate_normals_accepts_arrays_and_clouds(fp):
    class Cloud(object):
        def __init__(self, points):
            self.points, self.normals = points, None

    c = ofp.case("C")
    f = fp.FPFH(0.15, 0.3)
    n = f.estimate_normals(c["points"])
    cloud = Cloud(c["points"].tolist())
    m = f.estimate_normals(cloud)
    assert n.shape == (c["points"].shape[0], 3) and n.tobytes() == m.tobytes() and cloud.normals is m
    # equal neighbour sets give bit-identical normals: a repeated point and its original
    both = c["normal_lists"][2][:20] >= 3
    assert np.array_equal(n[:20][both], n[600:620][both])


def test_abi_call_order_and_bounds(fp):
    from probreg_amd import _lib

    plan = fp.FpfhPlan()
    with pytest.raises(_lib.ProbregHipError):
        plan.search(fp.SEARCH_NORMALS, 0.1, 30)  # no data
    plan.set_data(ofp.cloud_c())
    with pytest.raises(_lib.ProbregHipError):
        plan.compute_normals()  # no search
    for which, radius, k in ((2, 0.1, 30), (0, 0.0, 30), (0, np.inf, 30), (0, 0.1, 0), (0, 0.1, fp.max_neighbours() + 1)):
        with pytest.raises(ValueError):
            plan.search(which, radius, k)
    plan.search(fp.SEARCH_FEATURES, 0.3, fp.max_neighbours())  # the longest list: all 80 neighbours fit
    assert np.array_equal(plan.neighbours(fp.SEARCH_FEATURES)[2], ofp.hybrid_search(ofp.cloud_c(), 0.3, 512)[2])
    with pytest.raises(_lib.ProbregHipError):
        plan.compute_spfh()  # no normals
    plan.close()


def test_filterreg_with_fpfh_features_matches_the_restatement_as_callable(fp):
    from probreg_amd import filterreg, synthetic

    src, tgt, _ = synthetic.filterreg_pair(600)
    kw = dict(sigma2=1000, maxiter=2, tol=-1)
    a = filterreg.registration_filterreg(src, tgt, feature_fn=fp.FPFH(0.15, 0.3), **kw)
    b = filterreg.registration_filterreg(src, tgt, feature_fn=fp.FPFH(0.15, 0.3), **kw)
    ref = filterreg.registration_filterreg(src, tgt, feature_fn=ofp.Restatement(0.15, 0.3), **kw)
    assert a.transformation.rot.tobytes() == b.transformation.rot.tobytes()
    assert a.transformation.t.tobytes() == b.transformation.t.tobytes()
    er = np.max(np.abs(a.transformation.rot - ref.transformation.rot))
    et = np.max(np.abs(a.transformation.t - ref.transformation.t))
    print("FilterReg with FPFH: rot %.3g, t %.3g" % (er, et))
    assert er <= 1.0e-4 and et <= 1.0e-4
