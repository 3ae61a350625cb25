"""include/kshost.h's sixth audit pass from C: tests/cabi_usage_audit_hostfit.c -- solve, the six audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; one pod under a hostname spread claimed on a later existing node; the refusal -- as C99 with -Wall -Werror -pedantic, linked against the
emulator build of the two libraries (CPU) and against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_hostfit_cases as HC
import audit_topo_cases as TC


def _c_program(tmp_path, libdir):
    pr = HC._problem([TC._pod("s%d" % i, app="s", spread=HC._spread(4, "s")) for i in range(3)],      # three pods under one self-selecting hostname spread, maxSkew 4 ...
                     [TC._roomy("e0", TC.Z1), TC._roomy("e1", TC.Z2)])                                    # ... and two roomy existing nodes: first fit puts all three on e0
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_hostfit", pr, "1", "1")
    assert "genuine: 0 + 0 + 0 + 0 + 0 + 0 of 3 pods, 0 nodes flagged, truncated 1 -> act\n" in out, out
    assert "the fourth pass examined 0 pods, the sixth 3\n" in out, out
    # one class against e0 (3 + self <= 4), e1 and the template: one count test each
    assert "evaluated: 3 placed pods, 3 pods examined, 0 skipped, 1 eligible groups, 0 skipped, 3 pairs, 3 count tests, 3 pairs admitting\n" in out, out
    assert "claimed back: 3 rows, 0 pods flagged, truncated 0\n" in out, out
    assert "pod 1 claimed on node 1 instead of 0: 1 pods flagged, the pod carries 65536 -> solve in Go\n" in out, out
    assert "no commit numbers: -1\n" in out, out


def test_audit_hostfit_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_hostfit_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
