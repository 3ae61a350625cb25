"""include/kshost.h's third audit pass from C: tests/cabi_usage_audit_spread.c -- solve, the three audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; two of them exchanged; the refusal -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and
against the HIP ones (GPU)."""
import os
import subprocess
import sys

import pytest

import audit_spread_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_audit_spread")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_audit_spread.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    f = tmp_path / "problem.ksp"
    f.write_text(SC.zonal(6).to_ksp())      # six pods under a zonal spread with maxSkew 1 on labelled existing nodes: zones 1 2 3 1 2 3 in commit order
    out = subprocess.run([exe, str(f), "2", "3"], capture_output=True, text=True, timeout=600)      # the fourth pod (zone 1) before the third (zone 3): zone 1 chosen at 1 1 0
    assert out.returncode == 0, out.stdout + out.stderr
    assert "genuine: 0 + 0 + 0 of 6 pods, 0 nodes flagged, truncated 1 -> act\n" in out.stdout, out.stdout
    assert "evaluated: 6 placed pods, 6 pairs, 6 of them exactly, 0 spread groups unattempted\n" in out.stdout, out.stdout
    assert "claimed back: 6 rows, 0 pods flagged, truncated 0\n" in out.stdout, out.stdout
    assert "commit numbers exchanged: 1 pods flagged, the pod that went first carries 2048, the other 0 -> solve in Go\n" in out.stdout, out.stdout
    assert "no commit numbers: -1\n" in out.stdout, out.stdout


def test_audit_spread_from_c_on_the_emulator(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_audit_spread_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
