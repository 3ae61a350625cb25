"""include/ksolve.h's and include/kshost.h's audit calls from C: tests/cabi_usage_audit.c -- solve, audit, gate; a claimed result with one edit; the refusals -- as C99
with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and against the HIP ones (GPU)."""
import os
import subprocess
import sys

import pytest

import audit_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_audit")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_audit.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    f = tmp_path / "problem.ksp"
    f.write_text(C.tamper_problem().to_ksp())
    out = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    P, nodes = len(C.PODS), 4 + 2
    assert "before a solve: -1\n" in out.stdout, out.stdout
    assert f"genuine: 0 of {P} pods, 0 of {nodes} nodes flagged -> act\n" in out.stdout, out.stdout
    assert "claimed: 1 pods flagged, pod 0 carries 2 (1 with KS_AUDIT_POD_UNSCHEDULED_LIST), 0 nodes flagged -> solve in Go\n" in out.stdout, out.stdout
    assert "too many nodes claimed: -1\n" in out.stdout, out.stdout
    assert f"handle, totals only: {P} pods {nodes} nodes, 0 + 0 flagged, truncated 3\n" in out.stdout, out.stdout
    assert "handle, with tables: truncated 0, 0 + 0 flagged\n" in out.stdout, out.stdout


def test_audit_from_c_on_the_emulator(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_audit_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
