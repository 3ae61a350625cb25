"""include/kshost.h's fourth audit pass from C: tests/cabi_usage_audit_firstfit.c -- solve, the four audits, gate; the commit numbers read through ksh_placement_rows
and audited back as claimed; one pod claimed on a later existing node; the refusal -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two
libraries (CPU) and against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_topo_cases as TC


def _c_program(tmp_path, libdir):
    pr = TC.plain(3, True)      # three pods under no constraint and one roomy existing node ...
    pr.nodes = pr.nodes + [TC._roomy("e1", TC.Z2)]      # ... and a second one: first fit puts all three on e0
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_firstfit", pr, "1", "1")
    assert "genuine: 0 + 0 + 0 + 0 of 3 pods, 0 nodes flagged, truncated 1 -> act\n" in out, out
    assert "evaluated: 3 placed pods, 3 pods examined, 0 skipped, 3 pairs, 3 of them admitting\n" in out, out      # one class against e0, e1 and the template
    assert "claimed back: 3 rows, 0 pods flagged, truncated 0\n" in out, out
    assert "pod 1 claimed on node 1 instead of 0: 1 pods flagged, the pod carries 4096 -> solve in Go\n" in out, out
    assert "no commit numbers: -1\n" in out, out


def test_audit_firstfit_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_firstfit_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
