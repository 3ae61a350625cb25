"""include/kshost.h's third audit pass from C: tests/cabi_usage_audit_spread.c -- solve, the three audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; two of them exchanged; the refusal -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and
against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_spread_cases as SC


def _c_program(tmp_path, libdir):
    # six pods under a zonal spread with maxSkew 1 on labelled existing nodes: zones 1 2 3 1 2 3 in commit order
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_spread", SC.zonal(6), "2", "3")      # the fourth pod (zone 1) before the third (zone 3): zone 1 chosen at 1 1 0
    assert "genuine: 0 + 0 + 0 of 6 pods, 0 nodes flagged, truncated 1 -> act\n" in out, out
    assert "evaluated: 6 placed pods, 6 pairs, 6 of them exactly, 0 spread groups unattempted\n" in out, out
    assert "claimed back: 6 rows, 0 pods flagged, truncated 0\n" in out, out
    assert "commit numbers exchanged: 1 pods flagged, the pod that went first carries 2048, the other 0 -> solve in Go\n" in out, out
    assert "no commit numbers: -1\n" in out, out


def test_audit_spread_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_spread_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
