"""include/kshost.h's fifth audit pass from C: tests/cabi_usage_audit_limits.c -- solve, the five audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; the two edits the first four passes are silent on (a machine billed to the limited provisioner past its budget, a node that lost an option
it must have); the refusal; a node table too short -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and against
the HIP ones (GPU)."""
import os
import subprocess
import sys

import pytest

import audit_limits_cases as LC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_audit_limits")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_audit_limits.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    f = tmp_path / "problem.ksp"
    f.write_text(LC.capped_problem().to_ksp())      # `capped` (cpu 10) before `second`, five pods of 2500m: nodes 0 and 1 of capped, node 2 of second
    out = subprocess.run([exe, str(f), "2", "1", "2"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "genuine: 0 + 0 + 0 + 0 + 0 of 5 pods, 0 + 0 of 3 nodes flagged, truncated 3 -> act\n" in out.stdout, out.stdout
    assert "evaluated: 1 limited templates, 5 placed pods, 2 nodes, 5 pods, 1 pairs; 2 exact, 1 binding, 0 + 0 skipped\n" in out.stdout, out.stdout
    assert "claimed back: 5 rows, 0 pods and 0 nodes flagged, truncated 0\n" in out.stdout, out.stdout
    assert "node 2 billed to template 0: the other passes flag 0, this one 1 nodes, the node carries 256 -> solve in Go\n" in out.stdout, out.stdout
    assert "node 1 reduced to type 2: the other passes flag 0, this one 1 nodes, the node carries 512 -> solve in Go\n" in out.stdout, out.stdout
    assert "no commit numbers: -1\n" in out.stdout, out.stdout
    assert "a short node table: truncated 2, 1 nodes flagged\n" in out.stdout, out.stdout


def test_audit_limits_from_c_on_the_emulator(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_audit_limits_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
