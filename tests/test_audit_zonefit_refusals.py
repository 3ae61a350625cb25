"""What the audit's ninth pass refuses (include/kshost.h ksh_audit_zonefit / ksh_audit_zonefit_claimed, include/ksolve.h ks_audit_zonefit_dev / _batch_dev): the
refusals every pass shares (tests/audit_harness.py `refusals`: nothing solved, a table promised and not given, null arguments, more new nodes than max_new_nodes, no
commit numbers, a claimed result without arrays) and the totals alone with no table given -- on the emulator (CPU) and on the device (GPU).  A claimed result on a
derived view is KS_ERR_UNSUPPORTED: tests/test_audit_zonefit_gpu.py's derived batch asserts it."""
import pytest

import audit_harness as H

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import audit_harness as H, audit_zonefit_cases as ZC
H.refusals(ZC.D, S, ZC.tamper_problem(), ZC.refusal_totals)
print("RESULT " + json.dumps({"ok": True}))
"""


def test_refusals_on_the_emulator():
    assert H.run_emulated(CHILD) == {"ok": True}


@pytest.mark.gpu
def test_refusals():
    import audit_zonefit_cases as ZC
    from karpenter_core_amd import scheduler as S
    H.refusals(ZC.D, S, ZC.tamper_problem(), ZC.refusal_totals)
