"""include/kshost.h's eighth audit pass from C: tests/cabi_usage_audit_reasons.c -- solve and ksh_audit_reasons over the resident result; the result's arrays audited
back as claimed; one nibble of an unscheduled pod tampered, which the first pass lets through and the pass flags; the refusal of a claimed result without pod_reason
-- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_reasons_cases as RC


def _c_program(tmp_path, libdir):
    pr = RC.tamper_problem()
    pod = [p.uid for p in pr.pods].index("giant-0000")      # no type holds it: [7 2 7 7] over the open, the tainted, the zoned and the capped provisioner
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_reasons", pr, str(pod))
    assert "genuine: reasons 0 of %d pods flagged, truncated 1 -> record the events\n" % len(pr.pods) in out, out
    assert "evaluated: 17 placed pods, 25 of 25 unscheduled pods examined, 0 skipped; nibbles: 70 exact, 30 bounded, 0 not examined; 19 classes, 76 pairs\n" in out, out
    assert "claimed back: 0 pods flagged, truncated 0\n" in out, out
    assert "pod %d claimed with reason 5 instead of 7 for the first template: first pass 0 pods flagged, reasons 1 pods flagged, the pod carries %d -> solve in Go\n" % (pod, RC.B["REASON_STATIC"]) in out, out
    assert "no pod_reason: -1 claimed result: null array pod_reason\n" in out, out


def test_audit_reasons_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_reasons_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
