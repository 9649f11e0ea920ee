"""The text of the single-thread pose solves on the host, with no GPU: tests/host/pose_check.cpp includes csrc/small_linalg.h
(jacobi_svd), csrc/kabsch_pose.h and csrc/cpd_mstep.h, is built with the host C++ compiler under AddressSanitizer and UBSan
(their runtimes linked in statically), not linked against the HIP runtime, and run as a program of its own.  It is fed the
cross-covariances and moment blocks of every family of tests/oracle_pose.py and must satisfy what tests/test_pose_solves_gpu.py
asserts of the GPU: rotation entries within max(8 K_ref eps cond, 1e-12) of the NumPy restatement wherever the rotation is
unique; orthonormal, proper, finite and optimal everywhere; scale, sigma2 and q within 1e-12; the identity, bit for bit, on a
zero matrix; the affine solve singular exactly where the reference raises.  On top of that U and V of jacobi_svd are
orthonormal to 64 eps in every rank branch, and U diag(sv) V^T gives the matrix back.

The host compiler does not contract a * b + c, the device compiler does under -ffp-contract=on: what is measured here is the
text, not the device's bits."""
import os
import subprocess

import numpy as np
import pytest

import oracle_pose as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = sorted(op.FAMILIES)
FAMILIES_3D = [f for f in FAMILIES if op.cases(f)[0]["d"] == 3]
AFFINE_SINGULAR = {"planar_axis", "planar_oblique", "collinear", "coincident", "d2_collinear", "d2_coincident"}


@pytest.fixture(scope="module")
def pose_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pose_host") / "pose_check")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    # -Wno-unknown-pragmas: the device text asks for `#pragma unroll`, which the host compiler does not know
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unknown-pragmas",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           os.path.join(ROOT, "tests", "host", "pose_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert built.returncode == 0, built.stdout

    def run(records):
        """records: lists of [tag, numbers ...] -> one array of doubles per record."""
        text = "\n".join(" ".join(v if isinstance(v, str) else (str(v) if isinstance(v, int) else float(v).hex()) for v in r)
                         for r in records) + "\n"
        done = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert done.returncode == 0, done.stdout
        lines = done.stdout.strip().split("\n")
        assert lines[-1] == "pose_check ok %d" % len(records), done.stdout
        return [np.array([float(v) for v in line.split()[1:]]) for line in lines[:-1]]

    return run


def _pad3(a):
    out = np.zeros((3, 3))
    out[:a.shape[0], :a.shape[1]] = a
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_jacobi_svd_factors_every_rank_branch(pose_check, family):
    todo = [(c, lab, a, d) for c in op.cases(family) for lab, a, d, _ in op.case_matrices(c)]
    got = pose_check([["SVD", d] + list(_pad3(a).ravel()) for _, _, a, d in todo])
    for (c, lab, a, d), out in zip(todo, got):
        what = "%s %s" % (c["name"], lab)
        u, v, sv = out[:9].reshape(3, 3), out[9:18].reshape(3, 3), out[18:21]
        s1 = float(np.linalg.svd(a, compute_uv=False)[0])
        eu = float(np.max(np.abs(u.T @ u - np.identity(3))))
        ev = float(np.max(np.abs(v.T @ v - np.identity(3))))
        back = float(np.max(np.abs((u * sv) @ v.T - _pad3(a))))
        kept = int(np.count_nonzero(sv[:d] > op.RANK_RULE * np.max(sv))) if s1 > 0.0 else 0
        print("%-36s kept %d of %d columns: |U^T U - I| %.1e, |V^T V - I| %.1e, |U S V^T - a| / s1 %.1e"
              % (what, kept, d, eu, ev, back / s1 if s1 > 0.0 else 0.0))
        assert np.all(np.isfinite(out))
        assert eu <= op.ORTHO and ev <= op.ORTHO, what
        assert back <= op.ORTHO * s1, what
        rank = op.claims(c)[0]
        assert kept == (2 if c["base"] == "planar_noise_1e-9" else rank), what  # the branch the family is there for
        assert np.allclose(np.sort(sv[:d])[::-1], np.linalg.svd(a, compute_uv=False), rtol=0.0, atol=op.ORTHO * s1), what
        if d == 2:
            assert np.array_equal(u[2], [0.0, 0.0, 1.0]) and np.array_equal(u[:, 2], [0.0, 0.0, 1.0]) and sv[2] == 0.0, what


@pytest.mark.parametrize("family", FAMILIES_3D)
def test_kabsch_pose_on_every_family(pose_check, family):
    """kabsch_pose is 3-D only; a cpd cross-covariance is handed over transposed (its kabsch rotation is the cpd one)."""
    worst = op.Worst()
    rng = np.random.default_rng(5)
    todo = []
    for c in op.cases(family):
        for lab, a, d, conv in op.case_matrices(c):
            hm = a if conv == "kabsch" else a.T
            scale = c["scale"]
            todo.append((c, lab, hm, rng.integers(-50, 51, size=3) * scale, rng.integers(-50, 51, size=3) * scale))
    got = pose_check([["KABSCH"] + list(hm.ravel()) + list(pm) + list(qm) for _, _, hm, pm, qm in todo])
    for (c, lab, hm, pm, qm), out in zip(todo, got):
        what = "%s %s" % (c["name"], lab)
        rot, t = out[:9].reshape(3, 3), out[9:]
        bound = op.check_rotation(rot, hm, 3, "kabsch", family, what, worst, "kabsch_pose")
        if not np.any(hm):
            assert np.array_equal(rot, np.identity(3)) and np.array_equal(t, qm - pm), what
        assert np.all(np.isfinite(t))
        # t = qm - R pm with the rotation the solve returned, and against the restatement where that is unique
        assert np.max(np.abs(t - (qm - rot @ pm))) <= 16.0 * op.EPS * max(np.max(np.abs(pm)), np.max(np.abs(qm))), what
        if op.describe(hm, 3)["unique"]:
            t_ref = op.pose(hm, pm, qm, 3, "kabsch")[1]
            assert np.max(np.abs(t - t_ref)) <= bound * max(1.0, np.max(np.abs(pm)), np.max(np.abs(qm))), what
    print("worst: " + worst.report())


def test_rank_one_rotation_is_a_continuous_function_of_the_matrix(pose_check):
    """On a rank-1 cross-covariance the rotation about the one direction the data fix is free, and it must not be left to
    round-off: the batched and the single CPD path hand the M-step moments that differ in the last bits, and their rotations
    of a collinear problem were 4e-3 .. 0.5 apart while V's null columns came out of the sweeps as they fell.  A relative
    perturbation of 1e-9 (with 1e-17 of full-rank noise on top) may move the rotation by 1e-9 times a modest factor."""
    rng = np.random.default_rng(3)
    u, x = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), np.array([0.3, -1.2, 0.7])
    mats = [np.outer(u, x)] + [np.outer(u * (1.0 + 1e-9 * rng.normal(size=3)), x * (1.0 + 1e-9 * rng.normal(size=3)))
                              + 1e-17 * rng.normal(size=(3, 3)) for _ in range(8)]
    zero = [0.0] * 3
    poses = pose_check([["KABSCH"] + list(m.ravel()) + zero + zero for m in mats])
    params = pose_check([["MSTEP", 0, 0, 3, 1.0] + zero + zero + list(m.ravel()) + [1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 3.0] + [0.0] * 9
                         for m in mats])
    for name, rots in (("kabsch_pose", [p[:9] for p in poses]), ("mstep_body", [p[:9] for p in params])):
        moved = max(float(np.max(np.abs(r - rots[0]))) for r in rots[1:])
        print("%s: a 1e-9 perturbation of a rank-1 matrix moves the rotation by %.2e" % (name, moved))
        assert moved <= 1.0e-7, name
        for r in rots:
            orth, det, finite = op.invariants(r.reshape(3, 3))
            assert finite and orth <= op.ORTHO and det <= op.ORTHO


def _rigid_fields(params, d):
    return dict(rot=params[:9].reshape(3, 3), t=params[9:12], scale=params[12], sigma2=params[13], q=params[14])


@pytest.mark.parametrize("update_scale", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_rigid_mstep_on_every_family(pose_check, family, update_scale):
    worst = op.Worst()
    todo = [(c, kind, op.cpd_moments(c["src"], c["tgt"], c["p"][kind])[0]) for c in op.cases(family) for kind in op.P_KINDS]
    got = pose_check([["MSTEP", 0, int(update_scale), c["d"]] + list(mom) for c, _, mom in todo])
    for (c, kind, mom), params in zip(todo, got):
        d = c["d"]
        what = "%s %s scale=%d" % (c["name"], kind, update_scale)
        g = _rigid_fields(params, d)
        a = op.cpd_cross_covariance(mom, d)
        ref = op.cpd_rigid(mom, d, update_scale)
        bound = op.check_rotation(g["rot"], a, d, "cpd", family, what, worst, "mstep_body rigid")
        if d == 2:
            assert np.array_equal(g["rot"][2], [0.0, 0.0, 1.0]) and np.array_equal(g["rot"][:, 2], [0.0, 0.0, 1.0]), what
            assert g["t"][2] == 0.0
        op.check_scalars(g, ref, what)
        assert params[15] == mom[0] and params[16] == 1.0
        mu_x, mu_y = mom[1:1 + d] / mom[0], mom[4:4 + d] / mom[0]
        if not np.any(a):
            assert np.array_equal(g["rot"], np.identity(3)), what
            if not update_scale:
                assert np.array_equal(g["t"][:d], mu_x - mu_y), what
        elif op.describe(a, d)["unique"]:
            centroid = max(1.0, float(np.max(np.abs(mu_x))), float(np.max(np.abs(mu_y))))
            assert np.max(np.abs(g["t"][:d] - ref["t"])) <= bound * centroid, what
    print("worst: " + worst.report())


def test_affine_mstep_is_singular_where_the_reference_raises(pose_check):
    todo = [(c, kind, op.cpd_moments(c["src"], c["tgt"], c["p"][kind])[0]) for c in op.all_cases() for kind in op.P_KINDS]
    got = pose_check([["MSTEP", 1, 1, c["d"]] + list(mom) for c, _, mom in todo])
    solved = set()
    for (c, kind, mom), params in zip(todo, got):
        d = c["d"]
        what = "%s %s" % (c["name"], kind)
        b = params[:9].reshape(3, 3)[:d, :d]
        if c["base"] in AFFINE_SINGULAR:
            with pytest.raises(np.linalg.LinAlgError):
                op.cpd_affine(mom, d)
            assert not np.all(np.isfinite(b)), what  # what the host maps to LinAlgError
            continue
        ref = op.cpd_affine(mom, d)
        bound = max(op.MARGIN * ref["disagreement"], op.TOL_FLOOR * ref["cond"])
        diff = float(np.max(np.abs(b - ref["b"])))
        print("%-40s |b - solve| %.2e, solve against lstsq %.2e, cond(YPY) %.2e, bound %.2e"
              % (what, diff, ref["disagreement"], ref["cond"], bound))
        assert np.all(np.isfinite(params[:16])) and diff <= bound, what
        solved.add(c["base"])
    assert "planar_noise_1e-5" in solved and "full" in solved and "d2_full" in solved


def test_supported_range_is_written_on_jacobi_svd():
    """The column norms are sums of squares: entries below about 1e-150 or above 1e150 leave the supported range, and the header
    says so where jacobi_svd is declared."""
    with open(os.path.join(ROOT, "probreg_amd", "csrc", "small_linalg.h")) as f:
        text = f.read()
    head = text[:text.index("inline void jacobi_svd")]
    assert "1e-150" in head and "1e150" in head
