"""include/kshost.h's second audit pass from C: tests/cabi_usage_audit_topology.c -- solve, both audits, gate; the commit numbers read through ksh_placement_rows and
audited back as claimed; two of them exchanged; the refusal -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries (CPU) and
against the HIP ones (GPU)."""
import pytest

import audit_harness as H
import audit_topo_cases as TC


def _c_program(tmp_path, libdir):
    P = len(TC.PODS)
    out = H.run_c_program(tmp_path, libdir, "cabi_usage_audit_topology", TC.tamper_problem(), str(TC.PODS.index("fol_h")), str(TC.PODS.index("lead")))
    assert f"genuine: 0 + 0 of {P} pods, 0 nodes flagged, truncated 1 -> act\n" in out, out
    assert f"evaluated: {P} commit numbers, anti-affinity yes, affinity yes, hostname spread yes, 0 groups skipped\n" in out, out
    assert f"claimed back: {P} rows, 0 pods flagged, truncated 0\n" in out, out
    assert "the leader was committed before the follower\n" in out, out
    assert "commit numbers exchanged: 1 pods flagged, the follower carries 512 (1 with KS_AUDIT_POD_AFFINITY) -> solve in Go\n" in out, out
    assert "no commit numbers: -1\n" in out, out


def test_audit_topology_from_c_on_the_emulator(tmp_path):
    _c_program(tmp_path, H.sim_libdir())


@pytest.mark.gpu
def test_audit_topology_from_c(tmp_path):
    _c_program(tmp_path, H.hip_libdir())
