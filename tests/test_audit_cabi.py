"""include/ksolve.h's and include/kshost.h's audit calls from C: tests/cabi_usage_audit.c -- solve, audit, gate; a claimed result with one edit; the refusals -- as C99
with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and against the HIP ones (GPU)."""
import pytest

import audit_cases as C
import audit_harness as H


def _c_program(tmp_path, libdir):
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit", C.tamper_problem())
    P, nodes = len(C.PODS), 4 + 2
    assert "before a solve: -1\n" in out, out
    assert f"genuine: 0 of {P} pods, 0 of {nodes} nodes flagged -> act\n" in out, out
    assert "claimed: 1 pods flagged, pod 0 carries 2 (1 with KS_AUDIT_POD_UNSCHEDULED_LIST), 0 nodes flagged -> solve in Go\n" in out, out
    assert "too many nodes claimed: -1\n" in out, out
    assert f"handle, totals only: {P} pods {nodes} nodes, 0 + 0 flagged, truncated 3\n" in out, out
    assert "handle, with tables: truncated 0, 0 + 0 flagged\n" in out, out


def test_audit_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
