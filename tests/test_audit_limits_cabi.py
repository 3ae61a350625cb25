"""include/kshost.h's fifth audit pass from C: tests/cabi_usage_audit_limits.c -- solve, the five audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; the two edits the first four passes are silent on (a machine billed to the limited provisioner past its budget, a node that lost an option
it must have); the refusal; a node table too short -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and against
the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_limits_cases as LC


def _c_program(tmp_path, libdir):
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_limits", LC.capped_problem(), "2", "1", "2")      # `capped` (cpu 10) before `second`, five pods of 2500m: nodes 0 and 1 of capped, node 2 of second
    assert "genuine: 0 + 0 + 0 + 0 + 0 of 5 pods, 0 + 0 of 3 nodes flagged, truncated 3 -> act\n" in out, out
    assert "evaluated: 1 limited templates, 5 placed pods, 2 nodes, 5 pods, 1 pairs; 2 exact, 1 binding, 0 + 0 skipped\n" in out, out
    assert "claimed back: 5 rows, 0 pods and 0 nodes flagged, truncated 0\n" in out, out
    assert "node 2 billed to template 0: the other passes flag 0, this one 1 nodes, the node carries 256 -> solve in Go\n" in out, out
    assert "node 1 reduced to type 2: the other passes flag 0, this one 1 nodes, the node carries 512 -> solve in Go\n" in out, out
    assert "no commit numbers: -1\n" in out, out
    assert "a short node table: truncated 2, 1 nodes flagged\n" in out, out


def test_audit_limits_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_limits_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
