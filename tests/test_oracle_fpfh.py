"""The FPFH restatement (tests/oracle_fpfh.py) against properties that need no GPU: the conditions the GPU comparisons of
test_fpfh_gpu.py rest on, the sums of the histograms, the closed form of a planar cloud and a brute-force search."""
import numpy as np
import pytest

import oracle_fpfh as ofp


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_no_point_of_the_test_clouds_is_fragile(name):
    """The condition of the exact comparisons on the GPU: no decision of any point is within 1e-7 of flipping."""
    c = ofp.case(name)
    assert ofp.MARGIN == 1.0e-7
    assert int(c["fragile"].sum()) == 0


def test_the_clouds_exercise_capped_uncapped_and_degenerate_lists():
    (_, _, na), (_, _, fa) = ofp.case("A")["normal_lists"], ofp.case("A")["feature_lists"]
    assert int((na < 3).sum()) == 10 and int((fa == 100).sum()) == 1478
    (_, _, nb), (_, _, fb) = ofp.case("B")["normal_lists"], ofp.case("B")["feature_lists"]
    assert int((nb == 30).sum()) > 1400 and fb.min() == 3 and fb.max() == 46
    c = ofp.case("C")
    (_, d2, nc), (_, _, fc) = c["normal_lists"], c["feature_lists"]
    assert int((nc < 3).sum()) == 20 and int((fc == 1).sum()) == 12
    assert int(((d2[:, 1] == 0.0) & (nc > 1)).sum()) == 40  # the 20 repeated points and their originals


@pytest.mark.parametrize("name", ["A", "B", "C", "P"])
def test_histogram_groups_sum_to_100_and_200(name):
    c = ofp.case(name)
    count = c["feature_lists"][2]
    lone = count <= 1
    for g in range(3):
        np.testing.assert_allclose(c["spfh"][~lone, 11 * g:11 * g + 11].sum(axis=1), 100.0, rtol=0, atol=1e-10)
        np.testing.assert_allclose(c["fpfh"][~lone, 11 * g:11 * g + 11].sum(axis=1), 200.0, rtol=0, atol=1e-9)
    assert not c["spfh"][lone].any() and not c["fpfh"][lone].any()
    assert c["fpfh"].shape == (count.shape[0], 33) and c["fpfh"].dtype == np.float64


def test_planar_cloud_gives_the_closed_form():
    c = ofp.case("P")
    assert c["normal_lists"][2].min() >= 3
    assert np.array_equal(c["normals"], np.tile([0.0, 0.0, 1.0], (500, 1)))
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(c["spfh"], np.tile(want, (500, 1)))
    assert np.array_equal(c["fpfh"], np.tile(2.0 * want, (500, 1)))


@pytest.mark.parametrize("radius,max_nn", [(0.15, 30), (0.3, 100), (10.0, 100), (0.3, 1), (0.3, 2)])
def test_search_agrees_with_brute_force(radius, max_nn):
    pts = ofp.cloud_c()
    got = ofp.hybrid_search(pts, radius, max_nn)
    want = ofp.hybrid_search_brute(pts, radius, max_nn)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_normals_are_unit_signed_and_report_their_gap():
    c = ofp.case("A")
    n, gap = c["normals"], c["gap"]
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, rtol=0, atol=1e-15)
    lead = np.argmax(np.abs(n), axis=1)
    assert np.all(n[np.arange(n.shape[0]), lead] > 0.0)
    default = c["normal_lists"][2] < 3
    assert np.array_equal(n[default], np.tile([0.0, 0.0, 1.0], (int(default.sum()), 1)))
    assert np.all(np.isinf(gap[default])) and 1.0e-4 < gap[~default].min() < 1.0
