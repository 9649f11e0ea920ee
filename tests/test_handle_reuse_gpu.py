"""One live handle, re-created in place: the FPFH plan, the mixture fit, the GMMTree plan and the one-class SVM each run
"cloud A, the smaller cloud B, cloud A again" on ONE handle, so every buffer group of the handle is released and
allocated again at another size, shrinks and grows back.  GPU against GPU on purpose (as
test_gmmtree_stages_gpu.test_reused_handle_gives_a_fresh_handles_bytes): these stages have no floating-point atomics, so

  * every output of the third run is byte-equal to the first run's, and
  * every output of the second run is byte-equal to the same calls on a fresh handle.

A = 300 points, B = 70 points: several cells of the search grid, several 64-point chunks, and component counts below
and above one 256-thread block.  What the stages compute is checked against the oracles by test_fpfh_gpu,
test_gmmfit_stages_gpu, test_gmmtree_stages_gpu and test_ocsvm_gpu; this file pins what re-creation must not change.

The other seven plan classes (the CPD plan, the CPD batch, the FilterReg plan, the stand-alone lattice, the RANSAC plan, the
voxel plan and the ICP plan) get the life cycle every handle shares (``_lib.Handle`` over csrc/plan_base.h) on a 64-point cloud
(the batch: 4 problems of 64): close twice; a device index one past the last is a ValueError that leaves no handle; a getter
before any data is the handle's own state error; and one tiny run on a handle created after the first was closed gives the
first run's bytes (none of these stages adds floating-point numbers in arrival order: the lattice splats in fixed point).
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


# ---- the life cycle of the other seven plan classes -------------------------------------------------------------------------
N_TINY = 64


def tiny_pair():
    from probreg_amd import synthetic

    src, tgt, _ = synthetic.rigid_pair(N_TINY, seed=41)
    return src, tgt


def check_lifecycle(cls, init, unset_getter, unset_message, run):
    """init(obj, device) constructs ``obj`` in place (device None: the current one); unset_getter(plan) reads a result that a
    new handle does not have; run(plan) -> [(name, array or scalar)] of one tiny run."""
    from probreg_amd import _lib

    def make():
        plan = cls.__new__(cls)
        init(plan, None)
        return plan

    plan = make()
    assert plan._h
    plan.close()
    assert not plan._h
    plan.close()
    refused = cls.__new__(cls)
    with pytest.raises(ValueError, match="out of range"):
        init(refused, _lib.device_count())
    assert not getattr(refused, "_h", None)
    refused.close()
    plan = make()
    try:
        with pytest.raises(_lib.ProbregHipError, match=unset_message) as info:
            unset_getter(plan)
        assert "status %d" % _lib.PRG_ERR_STATE in str(info.value)
        first = as_bytes(run(plan))
    finally:
        plan.close()
    again = make()
    try:
        second = as_bytes(run(again))
    finally:
        again.close()
    assert [o[0] for o in first] == [o[0] for o in second] and len(first) >= 1
    for a, b in zip(first, second):
        assert a == b, "%s differs on a handle created after the first was closed" % a[0]


def test_cpd_plan_lifecycle():
    from probreg_amd import _lib, engine

    src, tgt = tiny_pair()

    def run(plan):
        plan.set_source(src.astype(np.float32))
        plan.set_target(tgt.astype(np.float32))
        plan.init_sums()
        plan.init_params()
        plan.iterate(_lib.PRG_TF_RIGID, True, 0.1, 5)
        out = [("params", plan.get_params()), ("moments", plan.get_moments())]
        plan.estep(0.1)
        out += zip(("pt1", "p1", "px"), plan.get_estep())
        return out

    check_lifecycle(engine.CpdPlan, lambda p, d: p.__init__(device=d), lambda p: p.get_estep_pt1(),
                    "no E-step has been run", run)


def test_cpd_batch_plan_lifecycle():
    from probreg_amd import _lib, engine, synthetic

    pairs = [synthetic.rigid_pair(N_TINY, seed=50 + b)[:2] for b in range(4)]
    srcs = [s - s.mean(axis=0) for s, _ in pairs]
    tgts = [t - t.mean(axis=0) for _, t in pairs]

    def run(plan):
        plan.init()
        plan.iterate(_lib.PRG_TF_RIGID, True, np.full(4, 0.1), np.full(4, -1.0), 5)
        return list(zip(("params", "iterations"), plan.get_params()))

    check_lifecycle(engine.CpdBatchPlan, lambda p, d: p.__init__(srcs, tgts, device=d), lambda p: p.get_params(),
                    "prg_cpd_batch_init has not run", run)


def test_filterreg_plan_lifecycle():
    from probreg_amd import filterreg

    src, tgt = tiny_pair()

    def run(plan):
        plan.set_source(src)
        plan.set_target(tgt)
        plan.set_state(np.identity(3), np.zeros(3), 0.05)
        size, blur = plan.estep()
        out = [("lattice size", size), ("blur", blur), ("mstep", plan.mstep(0.1, True, "pt2pt", 1.0e-4)),
               ("state", plan.get_state())]
        out += zip(("m0", "m1", "m2"), plan.get_estep(True))
        return out

    check_lifecycle(filterreg._Plan, lambda p, d: p.__init__(device=d), lambda p: p.get_estep(False),
                    "no E-step has been run", run)


def test_permutohedral_lifecycle():
    from probreg_amd import _lib, gaussian_filtering as gf

    src, _ = tiny_pair()
    values = np.random.default_rng(7).uniform(0.0, 1.0, (N_TINY, 2))

    def init(plan, device):  # (the class builds its lattice in the constructor and takes no device: the handle alone)
        _lib.Handle.__init__(plan, _lib.lib.prg_ph_create, _lib.lib.prg_ph_destroy, device)

    def run(plan):
        plan.init(src / 0.2)
        return [("lattice size", plan.get_lattice_size()), ("filtered", plan.filter(values))]

    check_lifecycle(gf.Permutohedral, init, lambda p: p.get_lattice_size(), "lattice not initialised", run)


def test_ransac_plan_lifecycle():
    from probreg_amd import global_reg, synthetic

    p = synthetic.surface(N_TINY, 43)
    q = p @ synthetic.rot_zx(20.0, 10.0).T + np.array([0.1, -0.2, 0.05])

    def run(plan):
        plan.set_correspondences(p, q)
        plan.build(5, 256)
        out = list(zip(("triples", "pose", "valid"), plan.hypotheses()))
        plan.score(0.05)
        out += zip(("count", "sum"), plan.scores())
        best = plan.best()
        out += zip(("best index", "best count", "best sum", "best pose"), best)
        out += zip(("refined pose", "refined count", "refined sum", "inliers"), plan.refine(best[3], 0.05))
        return out

    check_lifecycle(global_reg.RansacPlan, lambda plan, d: plan.__init__(device=d), lambda plan: plan.scores(),
                    "prg_ransac_score first", run)


def test_voxel_plan_lifecycle():
    from probreg_amd import preprocess

    src, _ = tiny_pair()

    def run(plan):
        plan.set_data(src)
        plan.run(0.2)
        return [("count", plan.count()), ("keys", plan.keys()), ("order", plan.order()), ("rows", plan.rows()),
                ("means", plan.means()), ("counts", plan.counts()), ("first", plan.first()), ("inverse", plan.inverse())]

    check_lifecycle(preprocess.VoxelPlan, lambda p, d: p.__init__(device=d), lambda p: p.count(), "prg_voxel_run first", run)


def test_icp_plan_lifecycle():
    from probreg_amd import icp

    src, tgt = tiny_pair()

    def run(plan):
        plan.set_target(tgt)
        plan.set_source(src)
        plan.search(0.5)
        out = list(zip(("index", "d2"), plan.matches()))
        out += zip(("knn index", "knn d2", "knn count"), plan.knn(4))
        plan.iterate("point_to_point", 0.5, 5)
        state = plan.state()
        out += [("pose", state.pose), ("count", state.count), ("sum", state.sum), ("iterations", state.n_iter)]
        return out

    check_lifecycle(icp.IcpPlan, lambda p, d: p.__init__(device=d), lambda p: p.matches(), "no target", run)
