"""How a grid-mode matrix-core column launch deals the streamed chunks to its S segments (csrc/cpd_sweeps_mfma.hip,
k_colpass_mfma): contiguous runs (PRG_MFMA_DEAL=0) against chunk c -> segment c mod S (PRG_MFMA_DEAL=1).  Both
deals must visit every chunk exactly once, evaluate the same pairs and give the same moments up to the order fp32 partials are
added in; with the knob unset an all-pairs launch is the contiguous one, bit for bit.

The knob is read once per process, so every setting runs in a fresh child process (this file, `--child`), one after the other,
each under its own time limit; the child runs all cases and prints one JSON line.

Cases: synthetic.rigid_pair(n, m=m, seed=17), n targets (owned: blocks of 512) against m sources (streamed: chunks of 256); what
the host's segment rule (mfma_chunks_per_seg) cuts the fused launch into:
    (n, m)            blocks  chunks  segments x chunks per segment
    (1500, 700)         3       3      3 x 1                    (owned count below / across a 512-point block, ragged last chunk)
    (4133, 9001)        9      36     18 x 2
    (6000, 16651)      12      66     22 x 3                    (more than 64 chunks)
    (4133, 9300)        9      37     19 x 2, the last one 1    (19 does not divide 37: the interleaved deal gives segment 18 one
                                                                 chunk and the others two; 18 | 36 and 22 | 66 above)
Two states per case: (a) the first E-step of the registration - every pair is needed; (b) an E-step from a state the
vector-pipe sweeps were warmed up to, where fewer than half of the n m pairs are evaluated - the matrix-core sweep culls.
Moments of two engines / deals from one state agree within 2e-6 N_p (tests/test_mfma_gpu.py's bound between engines)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1500, 700), (4133, 9001), (6000, 16651), (4133, 9300)]
MAX_WARM = 60


def _estep_record(plan):
    return dict(pairs=list(plan.pair_counts()), fused=plan.last_estep_fused(), engines=list(plan.last_estep_engines()),
                moments=[float(v) for v in plan.get_moments()[:23]])


def _child():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from probreg_amd import _lib, cpd, synthetic

    out = []
    for n, m in CASES:
        src, tgt, _ = synthetic.rigid_pair(n, m=m, seed=17)
        assert src.shape[0] == m and tgt.shape[0] == n
        reg = cpd.RigidCPD(src)
        reg._initialize(tgt)
        plan = reg._plan
        plan.set_dense_engine(2)
        plan.set_moments_only(1)
        rec = dict(n=n, m=m)
        # (a) the first E-step on the matrix cores, then the vector pipe from the same state
        state = plan.get_params()
        plan.estep(0.0)
        rec["a_mfma"] = _estep_record(plan)
        plan.set_dense_engine(0)
        plan.set_params(state)
        plan.estep(0.0)
        rec["a_valu"] = _estep_record(plan)
        # (b) warm up on the vector pipe until an E-step evaluates fewer than half of the pairs; the matrix cores from its state
        plan.mstep(_lib.PRG_TF_RIGID, True)
        rec["warm"] = -1
        for it in range(MAX_WARM):
            state = plan.get_params()
            plan.estep(0.0)
            if plan.pair_counts()[0] < 0.5 * float(n) * m:
                rec["warm"] = it
                break
            plan.mstep(_lib.PRG_TF_RIGID, True)
        rec["b_valu"] = _estep_record(plan)
        plan.set_dense_engine(2)
        plan.set_params(state)
        plan.estep(0.0)
        rec["b_mfma"] = _estep_record(plan)
        out.append(rec)
    print("DEAL_JSON " + json.dumps(out))


def _run_child(deal):
    env = dict(os.environ)
    env.pop("PRG_MFMA_DEAL", None)
    env.pop("PRG_MFMA_DEAL_BELOW", None)
    if deal is not None:
        env["PRG_MFMA_DEAL"] = str(deal)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, timeout=240)
    assert run.returncode == 0, (deal, run.returncode, run.stderr[-3000:])
    lines = [l for l in run.stdout.splitlines() if l.startswith("DEAL_JSON ")]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0][len("DEAL_JSON "):])


@pytest.fixture(scope="module")
def deals():
    """{knob: records of every case}, the children one after the other (a child that fails ends the fixture)."""
    out = {}
    for deal in (0, 1, None):
        out[deal] = _run_child(deal)
    return out


def _np_of(rec):
    return rec["a_valu"]["moments"][0]


def _diff(a, b):
    return float(np.max(np.abs(np.asarray(a["moments"]) - np.asarray(b["moments"]))))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_both_deals_visit_every_chunk_once_and_run_the_fused_sweep(deals, case):
    n, m = CASES[case]
    for deal in (0, 1, None):
        rec = deals[deal][case]
        assert (rec["n"], rec["m"]) == (n, m)
        assert rec["warm"] >= 0, "the warm-up never reached a state with fewer than half of the pairs"
        print("deal", deal, "case", (n, m), "a pairs", rec["a_mfma"]["pairs"], "b pairs", rec["b_mfma"]["pairs"], "of", float(n) * m,
              "warm-up iterations", rec["warm"])
        assert rec["a_mfma"]["pairs"][0] == float(n) * m
        for st in ("a_mfma", "b_mfma"):
            assert rec[st]["fused"] == 1 and rec[st]["engines"][0] == 1, (deal, st, rec[st])
        # (the matrix-core sweep culled - by whole chunks and (128 x 16) tiles, so it keeps more pairs than the vector pipe did)
        assert rec["b_mfma"]["pairs"][0] < float(n) * m
    for st in ("a_mfma", "b_mfma"):
        assert deals[0][case][st]["pairs"] == deals[1][case][st]["pairs"], st


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_moments_agree_between_the_deals_and_with_the_vector_pipe(deals, case):
    for st in ("a", "b"):
        n_p = deals[0][case][st + "_valu"]["moments"][0]
        d01 = _diff(deals[0][case][st + "_mfma"], deals[1][case][st + "_mfma"])
        d0v = _diff(deals[0][case][st + "_mfma"], deals[0][case][st + "_valu"])
        d1v = _diff(deals[1][case][st + "_mfma"], deals[1][case][st + "_valu"])
        print("case", CASES[case], "state", st, "N_p %.1f" % n_p, "deal 0 vs 1 %.3e" % d01, "deal 0 vs vector pipe %.3e" % d0v,
              "deal 1 vs vector pipe %.3e" % d1v, "bound %.3e" % (2e-6 * n_p))
        assert d01 < 2e-6 * n_p, st
        assert d0v < 2e-6 * n_p, st
        assert d1v < 2e-6 * n_p, st


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CASES)))
def test_an_all_pairs_launch_with_the_knob_unset_is_the_contiguous_deal_bit_for_bit(deals, case):
    auto, contiguous = deals[None][case]["a_mfma"], deals[0][case]["a_mfma"]
    assert auto["moments"] == contiguous["moments"]
    assert auto["pairs"] == contiguous["pairs"]


if __name__ == "__main__" and sys.argv[1:] == ["--child"]:
    _child()
