"""include/kshost.h's seventh audit pass from C: tests/cabi_usage_audit_stages.c -- solve, the gate and ksh_audit_stages beside it; the commit numbers read through
ksh_placement_rows and audited back as claimed; one pod claimed one stage on, which the gate lets through and the pass flags; the refusal -- as C99 with -Wall -Werror
-pedantic, linked against the emulator build of the two libraries (CPU) and against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_stages_cases as SC


def _c_program(tmp_path, libdir):
    pod = SC.PODS.index("team_a")      # on e0, the node its preference names, at stage 0
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_stages", SC.tamper_problem(), str(pod))
    assert "genuine: gate 0 findings, stages 0 of 9 pods flagged, truncated 1 -> act\n" in out, out
    assert "evaluated: 8 placed pods, 1 pods with an examined stage, 8 skipped, 1 stages, 3 pairs, 0 of them admitting\n" in out, out      # giant's first stage against e0, e1 and the template
    assert "claimed back: 9 rows, 0 pods flagged, truncated 0\n" in out, out
    assert "pod %d claimed at stage 1 instead of 0: gate 0 findings, stages 1 pods flagged, the pod carries %d -> solve in Go\n" % (pod, SC.B["STAGE_EXISTING"]) in out, out
    assert "no commit numbers: -1\n" in out, out


def test_audit_stages_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_stages_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
