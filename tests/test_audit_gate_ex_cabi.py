"""include/kshost.h's wide audit gate from C: tests/cabi_usage_audit_gate_ex.c -- solve, ONE ksh_audit_gate_ex call with all eight passes and no table, act; the
commit numbers read through ksh_placement_rows and the result gated back as claimed, pod_reason among its arrays; one pod claimed one relaxation stage on: the old
gate's six passes find nothing, the wide gate one finding, the seventh pass's, and the pass's own call agrees; a reason word on a placed pod, gated without commit
numbers: one finding, the eighth pass's; the growth rule and the refusals -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two
libraries (CPU) and against the HIP ones (GPU).  The problem is tests/audit_stages_cases.py's tamper problem."""
import pytest

import audit_harness as H
import audit_reasons_cases as RC
import audit_stages_cases as SC


def _c_program(tmp_path, libdir):
    pod, placed = SC.PODS.index("team_a"), SC.PODS.index("plain_a")      # on e0, the node its preference names, at stage 0 | on e0
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_gate_ex", SC.tamper_problem(), str(pod), str(placed))
    assert "genuine: 0 findings, truncated 0 -> act\n" in out, out
    assert "totals: 9 pods, 0 + 0 + 0 + 0 + 0 + 0 + 0 + 0 pods flagged\n" in out, out
    assert "the seventh pass examined 1 pods over 1 stages and 3 pairs; the eighth 1 of 1 unscheduled pods\n" in out, out      # (tests/test_audit_stages_cabi.py's figures: giant)
    assert "claimed back: 0 findings, truncated 0\n" in out, out
    assert "pod %d claimed at stage 1: the six passes find 0, the eight 1 -> solve in Go\n" % pod in out, out
    assert "finding 0: problem 0, pass 6, table 0, index %d, flags %d\n" % (pod, SC.B["STAGE_EXISTING"]) in out and "finding 1:" not in out, out
    assert "the record behind them untouched: 1\n" in out, out
    assert "the seventh pass's own call: 1 pods flagged, the pod carries %d; the gate's totals say 1\n" % SC.B["STAGE_EXISTING"] in out, out
    assert "a word on placed pod %d, no commit numbers: 1 findings: pass 7, index %d, flags %d\n" % (placed, placed, RC.B["REASON_PLACED"]) in out, out
    assert "a struct that ends before stages, bit 64: -1\n" in out and "the same struct, the six: 0\n" in out and "bit 256: -1\n" in out, out
    assert "bit 64 through the old gate: -1\n" in out and "no commit numbers for the seventh pass: -1\n" in out, out
    assert "no pod_reason for the eighth pass: -1\n" in out and "no pod_reason, the eighth pass not asked: 0\n" in out, out


def test_audit_gate_ex_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_gate_ex_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
