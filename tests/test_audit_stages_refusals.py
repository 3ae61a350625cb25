"""(CPU) Every refusal of the seventh audit pass's four entry points (include/kshost.h ksh_audit_stages / ksh_audit_stages_claimed; include/ksolve.h ks_audit_stages_dev /
ks_audit_stages_batch_dev) is the fourth pass's for the same call, code and message: tests/test_audit_refusals.py's calls, made for `firstfit` and for `stages` in one
process and compared case by case -- and the fourth pass's are the ones that file records.  Runs the emulator in a subprocess."""
import pytest

import audit_harness as H
import test_audit_refusals as TR

ANCHOR = "\nfor what in PASSES:\n"      # where that child begins to use its table of out structs: the seventh pass's is added to the table just before
CHILD = TR.CHILD.replace(ANCHOR, '\nOUT["stages"] = S._AuditStagesOut' + ANCHOR)


@pytest.fixture(scope="module")
def recorded():
    assert TR.CHILD.count(ANCHOR) == 1
    return H.run_emulated(CHILD, [["firstfit", "stages"], TR.ARRAYS])


def test_every_refusal_equals_the_fourth_passes(recorded):
    fourth = {k[len("firstfit/"):]: tuple(v) for k, v in recorded.items() if k.startswith("firstfit/")}
    mine = {k[len("stages/"):]: tuple(v) for k, v in recorded.items() if k.startswith("stages/")}
    assert len(mine) > 60 and set(mine) == set(fourth), sorted(set(mine) ^ set(fourth))
    wrong = {k: (mine[k], fourth[k]) for k in mine if mine[k] != fourth[k]}
    assert not wrong, wrong


def test_the_fourth_passes_are_the_recorded_ones(recorded):
    want = {case: (per["firstfit"] if isinstance(per, dict) else per) for case, per in TR.EXPECTED.items()}
    got = {k[len("firstfit/"):]: tuple(v) for k, v in recorded.items() if k.startswith("firstfit/")}
    assert got == {k: v for k, v in want.items() if v is not None}


def test_refusals_seen_through_the_binding():
    """tests/audit_harness.py's refusals(), through FlatProblem.audit_stages: nothing solved, tables promised and not given, the totals alone, too many new nodes, no
    commit numbers, null arrays."""
    got = H.run_emulated(BINDING_CHILD)
    assert got == {"ok": True}, got


BINDING_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import audit_harness as H, audit_stages_cases as SC
H.refusals(SC.D, S, SC.many_relaxed(2), totals=lambda o, f: o.checked[1] == 1 and o.checked[2] == 1 and o.checked[3] == 3 and o.skipped_pods == 1 and o.admitting_pairs == 0)      # two pods, both placed, one of them relaxed
print("RESULT " + json.dumps({"ok": True}))
"""
