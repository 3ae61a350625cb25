"""include/kshost.h's second audit pass from C: tests/cabi_usage_audit_topology.c -- solve, both audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; two of them exchanged; the refusal -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and
against the HIP ones (GPU)."""
import os
import subprocess
import sys

import pytest

import audit_topo_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_audit_topology")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_audit_topology.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    f = tmp_path / "problem.ksp"
    f.write_text(TC.tamper_problem().to_ksp())
    P = len(TC.PODS)
    out = subprocess.run([exe, str(f), str(TC.PODS.index("fol_h")), str(TC.PODS.index("lead"))], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"genuine: 0 + 0 of {P} pods, 0 nodes flagged, truncated 1 -> act\n" in out.stdout, out.stdout
    assert f"evaluated: {P} commit numbers, anti-affinity yes, affinity yes, hostname spread yes, 0 groups skipped\n" in out.stdout, out.stdout
    assert f"claimed back: {P} rows, 0 pods flagged, truncated 0\n" in out.stdout, out.stdout
    assert "the leader was committed before the follower\n" in out.stdout, out.stdout
    assert "commit numbers exchanged: 1 pods flagged, the follower carries 512 (1 with KS_AUDIT_POD_AFFINITY) -> solve in Go\n" in out.stdout, out.stdout
    assert "no commit numbers: -1\n" in out.stdout, out.stdout


def test_audit_topology_from_c_on_the_emulator(tmp_path):
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_audit_topology_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
