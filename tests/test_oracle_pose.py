"""The pose restatement (tests/oracle_pose.py) against itself, on the host: every family has the rank, sign, ties and
uniqueness it claims, keeps its distance from the two thresholds of the device text (the 1e-14 rank rule of jacobi_svd, the
1e-12 pivot rule of the affine M-step), and its two independent solves (NumPy SVD; Horn's quaternions / atan2) agree within
the bound the GPU tests use wherever the rotation is unique and reach the same optimum everywhere.  K_ref, the pooled
disagreement of the two solves in units of eps cond, is printed per family.

Margins.  A singular-value ratio is at least 1e3 away from 1e-14 as the construction defines it (oracle_pose.nominal_ratios:
rational arithmetic on the stored clouds).  The fp64 matrix a call site forms of ``planar_noise_1e-9`` cannot show its
1e-18: an oblique fp64 matrix carries about 1e-17 .. 1e-16 of round-off in its smallest singular value, whoever forms it.
That is still a factor 100 below the rule, and the fp64 matrices are held to "below 1e-15 or above 1e-11"."""
import numpy as np
import pytest

import oracle_pose as op

FAMILIES = sorted(op.FAMILIES)


def _outside(v, rule, margin):
    return v < rule / margin or v > rule * margin


def test_k_ref_per_family():
    for f in FAMILIES:
        print("K_ref %-20s %.3f" % (f, op.k_ref(f)))
        assert np.isfinite(op.k_ref(f)) and op.k_ref(f) < 64.0  # two backward-stable solves: a few eps cond


@pytest.mark.parametrize("family", FAMILIES)
def test_family_is_what_it_claims(family):
    for c in op.cases(family):
        rank, sign, unique = op.claims(c)
        for v in (c["src"], c["tgt"]):
            assert not v.flags.writeable
        # the source is a float32 cloud with a mean of exactly zero (or one repeated point): the library stores it unchanged
        centred = c["src"] - c["src"].mean(axis=0)
        assert np.array_equal(centred.astype(np.float32).astype(np.float64), centred)
        for label, a, d, conv in op.case_matrices(c):
            info = op.describe(a, d)
            what = "%s %s" % (c["name"], label)
            if c["base"] == "planar_noise_1e-9":
                assert op.exact_rank(a) == 3 and info["sv"][2] < 1.0e-15 * info["sv"][0], what
            else:
                assert op.exact_rank(a) == rank, what
            if sign in (1, -1):
                assert np.sign(float(op.exact_det(a))) == sign and info["c"] == sign, what
            if c["base"] in ("tied", "tied_mirrored"):
                assert np.max(info["sv"]) - np.min(info["sv"]) <= 4.0 * op.EPS * info["sv"][0], what
            elif rank == 3 and c["base"] == "mirrored":
                assert info["sv"][0] > 1.5 * info["sv"][1] > 1.5 * 1.5 * info["sv"][2], what  # distinct
            if c["base"] == "mirrored_slab":
                assert info["sv"][2] < 1.0e-4 * info["sv"][0], what
            if c["base"] in ("coincident", "d2_coincident"):
                assert not np.any(a), what
            assert info["unique"] == unique, what
            if unique:
                assert info["cond"] < 1.0e3, what


@pytest.mark.parametrize("family", FAMILIES)
def test_margins_to_the_rank_rule_and_the_pivot_rule(family):
    for c in op.cases(family):
        for kind in op.P_KINDS:
            what = "%s %s" % (c["name"], kind)
            nominal = op.nominal_ratios(c, kind)
            mom = op.cpd_moments(c["src"], c["tgt"], c["p"][kind])[0]
            formed = op.sv_ratios(op.cpd_cross_covariance(mom, c["d"]), c["d"])
            print("%-36s s_k / s_1: construction %s, as formed in fp64 %s"
                  % (what, ["%.1e" % v for v in nominal], ["%.1e" % v for v in formed]))
            assert all(_outside(v, op.RANK_RULE, 1.0e3) for v in nominal), what
            assert all(_outside(v, op.RANK_RULE, 10.0) for v in formed), what
            for vn, vf in zip(nominal, formed):
                assert (vn > op.RANK_RULE) == (vf > op.RANK_RULE), what
            piv = op.affine_pivots(op.cpd_ypy(mom, c["d"]))
            print("%-36s affine pivots / max |YPY|: %s" % (what, ["%.1e" % v for v in piv]))
            assert all(_outside(v, op.PIVOT_RULE, 1.0e2) for v in piv), what
        w = op.kabsch_weights(c)
        if w is not None:
            hm = op.kabsch_moments(c["src"], c["tgt"], w)[0]
            assert all(_outside(v, op.RANK_RULE, 1.0e3) for v in op.sv_ratios(hm, c["d"])), c["name"]


@pytest.mark.parametrize("family", FAMILIES)
def test_two_host_solves_agree(family):
    k = op.k_ref(family)
    for c in op.cases(family):
        for label, a, d, conv in op.case_matrices(c):
            what = "%s %s" % (c["name"], label)
            info = op.describe(a, d)
            # the second solve is checked exactly as a GPU result is, against the first
            op.check_rotation(op.rotation_second(a, d, conv), a, d, conv, family, what + " second")
            op.check_rotation(op.rotation_svd(a, d, conv), a, d, conv, family, what + " svd")
            o1 = op.optimum_of(a, op.rotation_svd(a, d, conv), d, conv)
            o2 = op.optimum_of(a, op.rotation_second(a, d, conv), d, conv)
            assert abs(o1 - o2) <= op.ORTHO * info["sv"][0], what
            if info["unique"]:
                assert k > 0.0
        # the scalars of the rigid M-step do not depend on which optimal rotation a solve returns
        for kind in op.P_KINDS:
            mom = op.cpd_moments(c["src"], c["tgt"], c["p"][kind])[0]
            for update_scale in (True, False):
                first = op.cpd_rigid(mom, c["d"], update_scale)
                second = op.cpd_rigid(mom, c["d"], update_scale, solve=op.rotation_second)
                op.check_scalars(second, first, "%s %s scale=%d" % (c["name"], kind, update_scale))


def test_affine_restatement_raises_where_the_reference_does():
    singular = {"planar_axis", "planar_oblique", "collinear", "coincident", "d2_collinear", "d2_coincident"}
    for c in op.all_cases():
        for kind in op.P_KINDS:
            mom = op.cpd_moments(c["src"], c["tgt"], c["p"][kind])[0]
            if c["base"] in singular:
                with pytest.raises(np.linalg.LinAlgError):
                    op.cpd_affine(mom, c["d"])
            else:
                r = op.cpd_affine(mom, c["d"])
                assert np.all(np.isfinite(r["b"])) and r["disagreement"] <= 1.0e-6 * np.max(np.abs(r["b"]))


def test_pose_translation_and_conventions():
    a = np.array([[4.0, 1.0, 0.5], [-1.0, 3.0, 0.25], [0.5, 0.0, 2.0]])
    mu_a, mu_b = np.array([1.0, 2.0, 3.0]), np.array([-1.0, 0.5, 2.0])
    r_cpd, t_cpd = op.pose(a, mu_a, mu_b, 3, "cpd")
    r_kab, t_kab = op.pose(a.T, mu_a, mu_b, 3, "kabsch")
    assert np.allclose(r_cpd, r_kab, atol=1e-15) and np.allclose(t_cpd, mu_b - r_cpd @ mu_a)
    assert np.allclose(t_cpd, t_kab, atol=1e-14)
    # the rotation maximises its trace form: every nearby rotation scores less
    best = op.optimum_of(a, r_cpd, 3, "cpd")
    rng = np.random.default_rng(0)
    for _ in range(20):
        w = rng.normal(size=3) * 1e-3
        k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        near = r_cpd @ (np.identity(3) + k + 0.5 * k @ k)
        assert op.optimum_of(a, near, 3, "cpd") < best
