"""include/kshost.h's audit gate from C: tests/cabi_usage_audit_gate.c -- solve, ONE ksh_audit_gate call with all six passes and no table, act; the commit numbers read
through ksh_placement_rows and the result gated back as claimed; one pod under a hostname spread claimed on a later existing node: one finding, the sixth pass's, and
the sixth pass's own call agrees; a table of one record where two are found; the refusals -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of
the two libraries (CPU) and against the HIP ones (GPU).  The problem is tests/test_audit_hostfit_cabi.py's."""
import pytest

import audit_harness as H
import audit_hostfit_cases as HC
import audit_topo_cases as TC


def _c_program(tmp_path, libdir):
    pr = HC._problem([TC._pod("s%d" % i, app="s", spread=HC._spread(4, "s")) for i in range(3)],      # three pods under one self-selecting hostname spread, maxSkew 4 ...
                     [TC._roomy("e0", TC.Z1), TC._roomy("e1", TC.Z2)])                                    # ... and two roomy existing nodes: first fit puts all three on e0
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_gate", pr, "1", "1")
    assert "genuine: 0 findings, truncated 0 -> act\n" in out, out
    assert "totals: 3 pods, 2 nodes, 0 + 0 + 0 + 0 + 0 + 0 pods and 0 + 0 nodes flagged\n" in out, out
    assert "the fourth pass examined 0 pods, the sixth 3: 3 pairs, 3 count tests, 3 pairs admitting\n" in out, out      # (tests/test_audit_hostfit_cabi.py's figures)
    assert "claimed back: 3 rows, 0 findings, truncated 0\n" in out, out
    assert "pod 1 claimed on node 1 instead of 0: 1 findings, truncated 0 -> solve in Go\n" in out, out
    assert "finding 0: problem 0, pass 5, table 0, index 1, flags 65536\n" in out and "finding 1:" not in out, out
    assert "the record behind them untouched: 1\n" in out, out
    assert "the sixth pass's own call: 1 pods flagged, the pod carries 65536; the gate's totals say 1\n" in out, out
    assert "two pods moved, a table of one: 2 findings, truncated 1, the first on pod 1, the second record untouched: 1\n" in out, out
    assert "no commit numbers: -1\n" in out and "no pass: -1\n" in out and "no table for four records: -1\n" in out, out


def test_audit_gate_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_gate_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
