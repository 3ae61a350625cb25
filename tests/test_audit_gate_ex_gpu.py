"""(GPU) The audit's wide gate on the device (include/ksolve.h ks_audit_gate_ex_dev / ks_audit_gate_ex_batch_dev: the reduce kernels of
karpenter_core_amd/csrc/ks_audit_reduce.inc behind the eight passes' own kernels, the seventh pass's six launches queued with no host wait) against the eight passes'
own calls over the same results (tests/audit_gate_ex_checks.py: every totals field, the findings in the stated order, `clean`, twice the same bytes, and over the six
the old gate's answer):
  a) the small workload the audit's GPU tests use, config3(140, 3, 1), with all eight passes and the sub-masks;
  b) the mixed batch -- relaxing, non-relaxing, empty, unscheduled pods -- forward and reversed;
  c) the two tamper matrices behind the recorder, and the silent edits under pass 6 and 7;
  d) the derived what-ifs of the stages cases as one batch;
  e) the shapes at which the tail can go wrong, and a findings cap that ends inside pass 6's records.
tests/test_audit_gate_ex.py runs the same kernels' source on the emulator."""
import pytest

import audit_gate_ex_checks as X
import audit_reasons_cases as RC
import audit_stages_cases as SC
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu


def test_the_small_workload_all_eight_passes_and_the_sub_masks():
    f = S.FlatProblem(W.config3(140, 3, 1))
    try:
        f.solve(decode=False)
        eight, g = X.gate_against_calls(S, [f])
        X.wide_as_old(S, [f])
        print({w: d[0]["ms"] for w, d in eight.items()}, g["ms"])
        assert g["clean"] and g["n_findings"] == 0 and list(g["passes"]) == list(S.AUDIT_GATE_ALL) and g["passes"]["stages"][0]["n_new"] == f.result_arrays()["n_new"]
        one = f.audit_gate(passes=list(S.AUDIT_GATE_ALL), cap_findings=0)      # the plain yes/no gate
        assert one["clean"] and not one["truncated"] and one["passes"] == {w: v[0] for w, v in g["passes"].items()}
        claimed = {k: v for k, v in f.result_arrays().items() if k != "key_value"}      # the genuine result claimed back: both side arrays in one upload
        X.gate_against_calls(S, [f], claimed, f.pod_seq(), masks=(None, ["audit", "stages", "reasons"], ["audit", "reasons"]))
    finally:
        f.close()


def test_a_mixed_batch_forward_and_reversed():
    got = X.mixed_batch_both_ways(S)
    print(got)
    assert got["stages"][0] > 0 and got["stages"][1:] == [0, 0, 0] and got["unscheduled"][3] > 0 and got["clean"] is True, got


@pytest.mark.parametrize("M", [SC, RC], ids=lambda M: M.__name__)
def test_the_tamper_matrices_behind_the_recorder(M):
    rec = X.Recorder(S, masks=(None,) + X.EX_MASKS)
    try:
        report = M.run_tamper_matrix(S)
    finally:
        rec.remove()
    bad = [r for r in report if r[1] is not True]
    assert not bad, bad[:3]      # (a difference between the gate and the eight calls is an AssertionError inside a pass's call: the matrix reports the case)
    print(M.__name__, len(rec.seen), sum(1 for s in rec.seen if s[4]))
    assert len(rec.seen) >= 8 and 0 < sum(1 for s in rec.seen if s[4]) < len(rec.seen), rec.seen


def test_the_silent_edits_are_listed_under_pass_six_and_seven():
    got = X.silent_edits(S)
    assert [e[1] for e in got] == [6] * 4 + [7] * 9 and all(len(e[2]) == 1 for e in got), got


def test_the_derived_whatifs_of_the_stages_cases_as_one_batch():
    rec = X.Recorder(S)
    try:
        plain, derived = SC.derived_whatifs(S)
    finally:
        rec.remove()
    print(len(rec.seen), [s[:2] for s in rec.seen if s[1] > 1])
    batches = [g for s, g in zip(rec.seen, rec.gates) if s[1] == len(SC.RELAX_WHATIF_SETS)]      # the flattened what-ifs as a batch, the derived ones as a batch
    assert len(batches) >= 2 and all(sum(d["checked"]["STAGES"] for d in g["passes"]["stages"]) > 0 and g["clean"] for g in batches), rec.seen


def test_the_shapes_at_which_the_tail_can_go_wrong_and_the_cap():
    assert [s[0] for s in X.tail_shapes(S)] == ["P = 1", "P = 257", "no pod relaxed at all", "M = 9"]
    n, n6, n7 = X.cap_inside_pass_six(S)
    assert n6 == 2 and n7 >= 1 and n == n6 + n7
