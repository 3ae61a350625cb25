"""(GPU) The audit's gate on the device (include/ksolve.h ks_audit_gate_dev / ks_audit_gate_batch_dev; the reduce kernels of karpenter_core_amd/csrc/ks_audit_reduce.inc
behind the six passes' own kernels) against the six passes' own calls over the same results (tests/audit_gate_checks.py: every totals field, the findings in the
stated order, `clean`, twice the same bytes):
  a) the small workload the audit's GPU tests use, config3(140, 3, 1), with all six passes and the three sub-masks;
  b) the six derived what-ifs of tests/audit_harness.py's WHATIF_SETS as one batch, and the same what-ifs flattened one by one;
  c) rr_problem(9013) with pod 810 claimed as the opener of an added node: the gate lists exactly the findings the sixth pass flags, HFIT_NEW on pod 810 among them;
  d) the tamper problems of each pass: the gate behind every call of each cases module's tamper matrix;
  e) findings at the cap.
tests/test_audit_gate.py runs the same kernels' source on the emulator."""
import numpy as np
import pytest

import audit_cases as AC
import audit_firstfit_cases as FC
import audit_gate_checks as G
import audit_harness as H
import audit_hostfit_cases as HC
import audit_limits_cases as LC
import audit_spread_cases as SC
import audit_topo_cases as TC
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu


def test_the_small_workload_all_six_passes_and_the_sub_masks():
    f = S.FlatProblem(W.config3(140, 3, 1))
    try:
        f.solve(decode=False)
        six, g = G.gate_against_calls(S, [f])
        print({w: d[0]["ms"] for w, d in six.items()}, g["ms"])
        assert g["clean"] and g["n_findings"] == 0 and g["passes"]["audit"][0]["n_new"] == f.result_arrays()["n_new"]
        one = f.audit_gate(cap_findings=0)      # the plain yes/no gate
        assert one["clean"] and not one["truncated"] and one["passes"] == {w: v[0] for w, v in g["passes"].items()}
    finally:
        f.close()


def test_the_derived_whatifs_as_one_batch():
    import test_whatif_derived as WD
    its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
    parsed = S.ParsedProblem(snap)
    flats = S.open_whatifs(parsed, pod_node, H.WHATIF_SETS, derive=False)
    S.solve_batch(flats, decode=False)
    derived = S.open_whatifs(parsed, pod_node, H.WHATIF_SETS, derive=True)
    S.solve_batch_resident(derived)
    try:
        six, g = G.gate_against_calls(S, derived)
        assert len(g["passes"]["hostfit"]) == len(H.WHATIF_SETS) and g["clean"]
        assert sum(d["checked"]["PODS"] for d in g["passes"]["hostfit"]) > 0 and sum(d["checked"]["SEQ"] for d in g["passes"]["topology"]) > 0
        plain = G.gate_against_calls(S, flats, masks=(None,))[1]
        assert plain["clean"] and [d["n_placed"] for d in plain["passes"]["spread"]] == [d["n_placed"] for d in g["passes"]["spread"]]
    finally:
        for f in flats + derived:
            f.close()


def test_rr_9013_pod_810_claimed_as_the_opener_of_an_added_node():
    import test_fuzz_rr as R
    f = S.FlatProblem(R.rr_problem(9013))
    rec = G.Recorder(S)
    try:
        f.solve(decode=False)
        h = HC.historical_case(S, f)      # (its two claimed calls, the sixth pass's and the first's, go through the recorder: the gate is compared behind both)
        print(h)
        assert h["ok"] is True and h["pod"] == HC.HISTORICAL_POD, h
        claimed = [g for s, g in zip(rec.seen, rec.gates) if s[2]]
        assert len(claimed) == 2
        sixth = [(int(x["problem"]), int(x["index"]), int(x["flags"])) for x in claimed[0]["findings"] if x["where"] >> 8 == 5]
        # (the recorder has already held the list against the sixth pass's own table, entry for entry: pod 810's is in it, with the pods the edit pushes over too)
        assert (0, HC.HISTORICAL_POD, HC.B["HFIT_NEW"]) in sixth and len(sixth) == 1 + h["others_flagged"], (sixth, h)
        assert claimed[0]["passes"]["hostfit"][0]["n_pods_flagged"] == len(sixth) and not claimed[0]["clean"]
    finally:
        rec.remove()
        f.close()


@pytest.mark.parametrize("M", [AC, TC, SC, FC, LC, HC], ids=lambda M: M.__name__)
def test_the_tamper_problems_of_each_pass(M):
    rec = G.Recorder(S)
    try:
        report = M.run_tamper_matrix(S)
    finally:
        rec.remove()
    bad = [r for r in report if r[1] is not True]
    assert not bad, bad[:3]      # (a difference between the gate and the six calls is an AssertionError inside a pass's call: the matrix reports the case)
    print(M.__name__, len(rec.seen), sum(1 for s in rec.seen if s[3]))
    assert len(rec.seen) >= 4 and 0 < sum(1 for s in rec.seen if s[3]) < len(rec.seen), rec.seen


def test_findings_at_the_cap():
    f = S.FlatProblem(SC.zonal(pods=640))
    try:
        f.solve(decode=False)
        r, s = G.all_flagged_claim(S, f)
        print(G.findings_at_the_cap(S, f, r, s))
    finally:
        f.close()
