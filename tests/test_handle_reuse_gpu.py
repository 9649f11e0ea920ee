"""One live handle, re-created in place: the FPFH plan, the mixture fit, the GMMTree plan and the one-class SVM each run
"cloud A, the smaller cloud B, cloud A again" on ONE handle, so every buffer group of the handle is released and
allocated again at another size, shrinks and grows back.  GPU against GPU on purpose (as
test_gmmtree_stages_gpu.test_reused_handle_gives_a_fresh_handles_bytes): these stages have no floating-point atomics, so

  * every output of the third run is byte-equal to the first run's, and
  * every output of the second run is byte-equal to the same calls on a fresh handle.

A = 300 points, B = 70 points: several cells of the search grid, several 64-point chunks, and component counts below
and above one 256-thread block.  What the stages compute is checked against the oracles by test_fpfh_gpu,
test_gmmfit_stages_gpu, test_gmmtree_stages_gpu and test_ocsvm_gpu; this file pins what re-creation must not change.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_A, N_B = 300, 70


def clouds():
    from probreg_amd import synthetic

    return synthetic.surface(N_A, 911), synthetic.surface(N_B, 912)


def as_bytes(outputs):
    return [(name, np.asarray(v).dtype.str, np.asarray(v).shape, np.ascontiguousarray(v).tobytes()) for name, v in outputs]


def check_reuse(make_plan, run):
    """run(plan, which) -> [(name, array or scalar)] for which in "A", "B"."""
    plan = make_plan()
    try:
        first, second, third = as_bytes(run(plan, "A")), as_bytes(run(plan, "B")), as_bytes(run(plan, "A"))
    finally:
        plan.close()
    fresh = make_plan()
    try:
        alone = as_bytes(run(fresh, "B"))
    finally:
        fresh.close()
    assert [o[0] for o in first] == [o[0] for o in third] and [o[0] for o in second] == [o[0] for o in alone]
    for a, b in zip(first, third):
        assert a == b, "%s of cloud A differs after the handle held cloud B" % a[0]
    for a, b in zip(second, alone):
        assert a == b, "%s of cloud B differs from a fresh handle's" % a[0]


def test_fpfh_plan():
    from probreg_amd import fpfh as fp

    a, b = clouds()

    def run(plan, which):
        plan.set_data(a if which == "A" else b)
        out = []
        plan.search(fp.SEARCH_NORMALS, 0.2, 30)
        out += zip(("normal idx", "normal d2", "normal count"), plan.neighbours(fp.SEARCH_NORMALS))
        plan.search(fp.SEARCH_FEATURES, 0.4, 100)
        out += zip(("feature idx", "feature d2", "feature count"), plan.neighbours(fp.SEARCH_FEATURES))
        plan.search(fp.SEARCH_FEATURES, 0.4, 40)      # the feature lists alone, shorter ...
        out += zip(("idx 40", "d2 40", "count 40"), plan.neighbours(fp.SEARCH_FEATURES))
        plan.search(fp.SEARCH_FEATURES, 0.4, 100)     # ... and long again
        out += zip(("idx again", "d2 again", "count again"), plan.neighbours(fp.SEARCH_FEATURES))
        assert [o[1].tobytes() for o in out[3:6]] == [o[1].tobytes() for o in out[9:12]]
        plan.compute_normals()
        out.append(("normals", plan.normals()))
        plan.compute_spfh()
        out.append(("spfh", plan.spfh()))
        plan.compute_fpfh()
        out.append(("fpfh", plan.fpfh()))
        counts = out[3][1].shape[0], int(out[5][1].min()), int(out[5][1].max())
        print("fpfh %s: %d points, feature lists of %d .. %d" % ((which,) + counts))
        return out

    check_reuse(fp.FpfhPlan, run)


def test_gmmfit_plan():
    from probreg_amd import features

    a, b = clouds()
    # components per cloud: below one block, then above it on the same data (the component group grows in place)
    ks = {"A": (40, 280), "B": (16, 60)}

    def run(plan, which):
        x = a if which == "A" else b
        plan.set_data(x)
        out = []
        for k in ks[which]:
            plan.seed(k, features.seed_uniforms(k, 7))
            out += [("seeds k=%d" % k, plan.seeds()), ("seed centres k=%d" % k, plan.centers())]
            n_iter = plan.lloyd(20, features.lloyd_tolerance(x))
            out += [("lloyd iterations k=%d" % k, n_iter), ("lloyd centres k=%d" % k, plan.centers())]
            plan.init_from_labels(1.0e-6)
            out += zip(("weights k=%d" % k, "means k=%d" % k, "covariances k=%d" % k), plan.params())
        return out

    check_reuse(features.GmmFitPlan, run)


def test_gmmtree_plan():
    from probreg_amd import gmmtree

    a, b = clouds()
    levels = {"A": 2, "B": 3}

    def run(plan, which):
        x, level = (a, levels["A"]) if which == "A" else (b, levels["B"])
        iters, q, dq = plan.build(x, level, gmmtree.init_indices(x.shape[0], level, 0), 0.001, 1.0e-4, 4)
        out = [("iterations", iters), ("q", q), ("dq", dq), ("nodes", plan.get_nodes())]
        plan.set_target(x)
        out += zip(("m01", "m2"), plan.reg_estep(np.identity(3), np.zeros(3), 1.0, 0.01, with_m2=True))
        return out

    check_reuse(gmmtree.GmmTreePlan, run)


def test_ocsvm_plan():
    from probreg_amd import svm

    a, b = clouds()

    def run(plan, which):
        x = a if which == "A" else b
        plan.set_data(x)
        out = list(zip(("rounds", "steps", "converged", "gap"), plan.solve(2.0, 0.2, 1.0e-5)))
        out += zip(("alpha", "rho", "objective", "support"), plan.solution())
        out.append(("decision", plan.decision(a[:50])))
        return out

    check_reuse(svm.OcsvmPlan, run)
