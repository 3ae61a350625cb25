"""CPU tests of the literal reference tests/deprovisioning_ref.py itself: Expiration / Drift.ComputeCommand over oracle/consolidation_ref.py's simulation WITH the
readiness rule of helpers.go:106-113, against `oracle/consolidation_ref.py::replacement_command`, which reads the simulation's new nodes without it.  The two agree on
the committed single-node scenarios and differ exactly where an owned, in-state node that stays is not initialised and the simulation opens a node."""

import pytest

from oracle import consolidation_ref as CR

import deprovisioning_ref as D
import test_consolidation as TC


def simulate(snapshot, i):
    sink = []
    CR.compute_consolidation(snapshot, [i], sink)      # raises ValueError for a candidate that is itself deleting
    return sink[0].new_nodes


def _both(snap, order):
    lit = D.replacement_command(snap, order, simulate)
    old = CR.replacement_command(snap, order)
    return (lit[0], lit[1], len(lit[2])), (old[0], old[1], len(old[2]))


@pytest.mark.parametrize("name", sorted(TC.scenarios()))
def test_agrees_with_the_existing_restatement_on_the_committed_scenarios(name):
    snap, cands, _ = TC.scenarios()[name]
    lit, old = _both(snap, list(range(len(snap.nodes))))
    assert lit == old and lit[0] in ("delete", "replace")


def _uninitialised_neighbour_that_cannot_help():
    """`can_replace_node` plus a second node with no room that is not initialised: the pod needs a new node, the neighbour stays."""
    snap, _, _ = TC.scenarios()["can_replace_node"]
    it = [t for t in snap.instance_types if t.name == snap.nodes[0].labels[TC.LABEL_INSTANCE_TYPE]][0]
    n2 = TC.node("n2", it, snap.nodes[0].labels[TC.LABEL_CAPACITY_TYPE], snap.nodes[0].labels[TC.LABEL_ZONE], cpu="0")
    del n2.labels["karpenter.sh/initialized"]
    snap.nodes.append(n2)
    snap.bound.append([])
    return snap


def test_differs_exactly_on_the_uninitialised_neighbour():
    lit, old = _both(_uninitialised_neighbour_that_cannot_help(), [0])
    assert old[0] == "replace" and old[2] >= 1          # the existing restatement reads the simulation's new nodes
    assert lit == ("delete", ["n1"], 0)                 # the reference: `return nil, false, nil`, then len(newNodes) == 0
    # with the neighbour initialised both say replace
    snap = _uninitialised_neighbour_that_cannot_help()
    snap.nodes[1].labels["karpenter.sh/initialized"] = "true"
    lit, old = _both(snap, [0])
    assert lit == old and lit[0] == "replace"


def test_deleting_candidates_are_passed_over_and_nobody_gives_do_nothing():
    snap, _, _ = TC.scenarios()["can_delete_nodes"]
    snap.deleting = (0,)
    got = D.replacement_command(snap, [0, 1], simulate)
    assert got[1] == ["n2"] and got[3] == 1
    assert D.replacement_command(snap, [0], simulate) == ("do-nothing", [], [], -1)
    assert D.replacement_command(snap, [], simulate) == ("do-nothing", [], [], -1)


# ---------------------------------------------------------------------------------------------------------------------
# The reference's own It()s (pkg/controllers/deprovisioning/suite_test.go), pinned by line and name: the literal candidates + ComputeCommand over the restated clusters of
# tests/test_consolidation.py::replacement_scenarios.
# ---------------------------------------------------------------------------------------------------------------------
import candidates_ref as R      # noqa: E402

NOW, S_NS = 1_700_000_000 * 10 ** 9, 10 ** 9


def _pass(method, scenario, ttl=None, created_ago=None, vd=None, drift_enabled=True):
    """One pass of the method over a scenario's snapshot: (command, candidates' dict)."""
    snap = TC.replacement_scenarios()[scenario][0]
    nodes = [D.DNode(labels=n.labels, pods=[R.RPod(k, "default", dict(p.labels)) for k, p in enumerate(b)], creation_ns=NOW - (created_ago[i] if created_ago else 0) * S_NS,
                     voluntary_disruption=(vd or {}).get(i)) for i, (n, b) in enumerate(zip(snap.nodes, snap.bound))]
    prov = D.DProvisioner("default", [it.name for it in snap.instance_types], True, ttl)
    c = D.candidates(method, nodes, [prov], [], NOW, drift_enabled)
    if c["n_in_result"] == 0:      # controller.go:167-170: the next method
        return ("do-nothing", [], [], -1), c
    return D.replacement_command(snap, c["order"], simulate), c


PINS = {
    (149, "should ignore drifted nodes if the feature flag is disabled"): lambda: _pass(D.DRIFT, "replace_one", vd={0: "drifted"}, drift_enabled=False),
    (182, "should ignore nodes with the drift label, but not the drifted value"): lambda: _pass(D.DRIFT, "replace_one", vd={0: "wrong-value"}),
    (214, "should ignore nodes without the drift label"): lambda: _pass(D.DRIFT, "replace_one"),
    (243, "can delete drifted nodes"): lambda: _pass(D.DRIFT, "delete_empty", vd={0: "drifted"}),
    (277, "can replace drifted nodes"): lambda: _pass(D.DRIFT, "replace_one", vd={0: "drifted"}),
    (332, "can replace drifted nodes with multiple nodes"): lambda: _pass(D.DRIFT, "replace_with_three", vd={0: "drifted"}),
    (424, "should delete one drifted node at a time"): lambda: _pass(D.DRIFT, "first_candidate_only", vd={0: "drifted", 1: "drifted"}),
    (474, "should ignore nodes without TTLSecondsUntilExpired"): lambda: _pass(D.EXPIRATION, "replace_one", ttl=None, created_ago=[10 ** 6]),
    (503, "can delete expired nodes"): lambda: _pass(D.EXPIRATION, "delete_empty", ttl=60, created_ago=[100]),
    (536, "should expire one node at a time, starting with most expired"): lambda: _pass(D.EXPIRATION, "first_candidate_only", ttl=60, created_ago=[100, 500]),
    (580, "can replace node for expiration"): lambda: _pass(D.EXPIRATION, "replace_one", ttl=60, created_ago=[100]),
    (725, "can replace node for expiration with multiple nodes"): lambda: _pass(D.EXPIRATION, "replace_with_three", ttl=60, created_ago=[100]),
}
WANT = {149: ("do-nothing", 0, (15, 0)), 182: ("do-nothing", 0, (15, 1)), 214: ("do-nothing", 0, (15, 1)), 243: ("delete", 0, None), 277: ("replace", 1, None), 332: ("replace", 3, None),
        424: ("delete", 0, None), 474: ("do-nothing", 0, (14, 0)), 503: ("delete", 0, None), 536: ("delete", 0, None), 580: ("replace", 1, None), 725: ("replace", 3, None)}


@pytest.mark.parametrize("line,title", sorted(PINS))
def test_the_reference_suite_is_pinned_by_name(line, title):
    (action, removed, new_nodes, pos), c = PINS[(line, title)]()
    want_action, want_new, want_code = WANT[line]
    assert (action, len(new_nodes)) == (want_action, want_new)
    if want_code:
        assert (c["why"][0], c["detail"][0]) == want_code and c["n_in_result"] == 0 and removed == []
    else:
        assert len(removed) == 1 and pos == 0           # one node at a time
    if line == 424:
        assert removed == ["to-expire"] and c["order"] == [0, 1]      # slot order: the canonical walk of the map
    if line == 536:
        assert c["order"] == [1, 0] and removed == ["not-yet"]        # created 500 s ago: the most expired, although the later slot
        assert _pass(D.EXPIRATION, "first_candidate_only", ttl=60, created_ago=[500, 100])[0][1] == ["to-expire"]
    if line in (332, 725):
        assert all(list(n.instance_types) == ["replacement-on-demand"] for n in new_nodes)
