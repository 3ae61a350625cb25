"""(CPU) Every refusal of the eighth audit pass's four entry points (include/kshost.h ksh_audit_reasons / ksh_audit_reasons_claimed; include/ksolve.h
ks_audit_reasons_dev / ks_audit_reasons_batch_dev) against the FIRST pass's for the same call, code and message: tests/test_audit_refusals.py's calls, made for `audit`
and for `reasons` in one process and compared case by case.  The two differ exactly where the issue says: the eighth pass reads pod_node, pod_stage and pod_reason
and nothing else, so a null array of any other name is accepted, and a null pod_reason is "claimed result: null array pod_reason" -- which the first pass, and
every other, accepts.  Runs the emulator in a subprocess."""
import pytest

import audit_harness as H
import test_audit_refusals as TR

# The eighth pass has the first pass's form -- no commit numbers -- under its own name: that child tells the two apart by `first`, which here stands for the form,
# while `alone` stands for the name.
EDITS = [('first = what == "audit"\n', 'first = what in ("audit", "reasons"); alone = what == "audit"\n'),
         ('name = "ksh_audit" if first else', 'name = "ksh_audit" if alone else'),
         ('getattr(ks, "ks_audit_dev" if first else', 'getattr(ks, "ks_audit_dev" if alone else'),
         ('getattr(ks, "ks_audit_batch_dev" if first else', 'getattr(ks, "ks_audit_batch_dev" if alone else'),
         ("\nfor what in PASSES:\n", '\nOUT["reasons"] = S._AuditReasonsOut\nfor what in PASSES:\n')]
READS = ("pod_node", "pod_stage", "pod_reason")


def _child():
    child = TR.CHILD
    for old, new in EDITS:
        assert child.count(old) == 1, old
        child = child.replace(old, new)
    return child


@pytest.fixture(scope="module")
def recorded():
    return H.run_emulated(_child(), [["audit", "reasons"], TR.ARRAYS])


def test_every_refusal_equals_the_first_passes_but_for_the_arrays_it_reads(recorded):
    first = {k[len("audit/"):]: tuple(v) for k, v in recorded.items() if k.startswith("audit/")}
    mine = {k[len("reasons/"):]: tuple(v) for k, v in recorded.items() if k.startswith("reasons/")}
    node_table = {"claimed/null node table, capacity 1", "resident/null node table, capacity 1"}      # the first pass has a table per node, this one has none
    assert len(mine) > 60 and set(mine) == set(first) - node_table, sorted(set(mine) ^ set(first))
    want = dict(first)
    for a in TR.ARRAYS:
        if a not in READS:
            want["claimed/null array " + a] = TR.ACCEPTED
    want["claimed/null array pod_reason"] = (-1, "claimed result: null array pod_reason")
    want["claimed/two at once: null node_it_state and null node_tmpl"] = TR.ACCEPTED      # neither is read
    wrong = {k: (mine[k], want[k]) for k in mine if mine[k] != want[k]}
    assert not wrong, wrong
    assert mine["claimed/two at once: null pod_node and null node_tmpl"] == first["claimed/two at once: null pod_node and null node_tmpl"] == (-1, "claimed result: null array")


def test_the_first_passes_are_the_recorded_ones(recorded):
    want = {case: (per["audit"] if isinstance(per, dict) else per) for case, per in TR.EXPECTED.items()}
    got = {k[len("audit/"):]: tuple(v) for k, v in recorded.items() if k.startswith("audit/")}
    assert got == {k: v for k, v in want.items() if v is not None}


def test_the_pass_refuses_only_the_arrays_it_reads(recorded):
    for a in TR.ARRAYS:
        assert (recorded["reasons/claimed/null array " + a][0] != 0) == (a in READS), (a, recorded["reasons/claimed/null array " + a])


def test_refusals_seen_through_the_binding():
    """tests/audit_harness.py's refusals(), through FlatProblem.audit_reasons: nothing solved, tables promised and not given, the totals alone, too many new nodes,
    null arrays."""
    got = H.run_emulated(BINDING_CHILD)
    assert got == {"ok": True}, got


BINDING_CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import audit_harness as H, audit_reasons_cases as RC
H.refusals(RC.D, S, RC.many_pods(4, 1), totals=lambda o, f: o.checked[0] == 1 and o.checked[1] == 1 and o.n_placed == 3 and o.n_unscheduled == 1 and o.skipped_pods == 0 and o.pairs == 1)      # four pods, one of them held by no type
print("RESULT " + json.dumps({"ok": True}))
"""
