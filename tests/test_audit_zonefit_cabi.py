"""include/kshost.h's ninth audit pass from C: tests/cabi_usage_audit_zonefit.c -- solve, the fourth, sixth and ninth pass; the commit numbers read through
ksh_placement_rows and audited back as claimed; one pod under a zonal spread claimed on a later existing node of its zone; the refusal -- as C99 with -Wall -Werror
-pedantic, linked against the emulator build of the two libraries (CPU) and against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_zonefit_cases as ZC


def _c_program(tmp_path, libdir):
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_zonefit", ZC.round_robin(6), "3", "3")      # six pods round the three zones; pod 3, on e0, claimed on e3
    assert "genuine: 0 + 0 + 0 of 6 pods flagged, truncated 1 -> act\n" in out, out
    assert "the fourth pass examined 0 pods, the sixth 0, the ninth 6\n" in out, out
    assert "evaluated: 6 placed pods, 6 pods examined, 0 skipped, 0 mixed, 1 eligible groups, 0 skipped, 36 zone tests, 24 passed, 24 pairs admitting, 6 pods exact\n" in out, out
    assert "claimed back: 6 rows, 0 pods flagged, truncated 0\n" in out, out
    assert "pod 3 claimed on node 3 instead of 0: 1 pods flagged, the pod carries 67108864 -> solve in Go\n" in out, out
    assert "no commit numbers: -1\n" in out, out


def test_audit_zonefit_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_zonefit_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
