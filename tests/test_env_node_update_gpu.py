"""NODE= (kshost.h KSH_EVENT_NODE_UPDATE) seen by the device paths.  The event has no kernel of its own: the kernels read whatever flattening they are given, so what
is checked here is that the flattening CONTINUED after node updates feeds them what a freshly ingested snapshot of the same objects feeds them --
  1. the derived what-ifs (ks_whatifs_open: per-node topology tables, volume state) solve like those over a fresh snapshot and like the oracle, after streams that move a
     zone label under bound spread pods and taint a node that would otherwise take a candidate's pods;
  2. the command kernel (ksh_consolidation_commands): an uninitialised node that stays blocks every command; the NODE= that initialises it unblocks them;
  3. the candidate kernels (ksh_consolidation_candidates): that node's reason goes from 6 to 0;
  4. the validation kernel (ksh_validate_commands): a delete stops being valid once the only node with room is tainted.
The shapes of 2 and 4 are checked on the reference restatement (oracle/consolidation_ref.py) first, without a device.  The CPU half is tests/test_env_node_update.py."""
import dataclasses
import json

import numpy as np
import pytest

from karpenter_core_amd import consolidation as C
from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import LABEL_PROVISIONER, LABEL_ZONE
from oracle import consolidation_ref as CR
from oracle import oracle_py as O

import test_consolidation as TC
from test_env_apply_block import make_cluster
from test_env_node_update import apply_through, model_after, stream

INIT = "karpenter.sh/initialized"
WHY_UNINITIALISED = 6


def plain(x):
    return json.loads(json.dumps(x))


# ---------------------------------------------------------------------------------------------------------------- 1. what-ifs
@pytest.mark.gpu
@pytest.mark.parametrize("seed,kind", [(41, "plain"), (42, "plain"), (43, "topology"), (44, "topology"), (45, "volumes"), (46, "volumes")])
def test_whatifs_after_node_updates_solve_like_a_fresh_snapshot(seed, kind):
    volumes = kind == "volumes"
    its, prov, nodes0, bound0, cps, make = make_cluster(kind, 28, 8, 500 + seed, spare_pod_slots=(6 if seed % 2 else -1))
    assert sum(len(b) for b in bound0) <= 300
    snap, pn = W.snapshot_problem(its, prov, nodes0, bound0, cps)
    parsed = S.ParsedProblem(snap)
    rs = np.random.RandomState(seed)
    for f in S.open_whatifs(parsed, pn, [[0], [1, 2]], derive=True, volumes=volumes):      # (flattened and resident BEFORE the events: they continue that flattening)
        f.close()
    after = model_after(kind)
    all_events, nodes, bound = [], nodes0, bound0
    for batch in range(2):
        events, nodes, bound = stream(kind, rs, its, nodes, bound, 12, f"u{seed}b{batch}", make)
        apply_through(parsed, "block" if batch else "text", events, pn if batch == 0 else None)
        all_events += events
    # a zone label moves under bound spread pods (their counts move to another domain) ...
    spread_on = [i for i, b in enumerate(bound) if any(p.spread for p in b) and nodes[i].labels.get(LABEL_PROVISIONER)]
    assert spread_on or kind != "topology"
    mover = spread_on[-1] if spread_on else max(i for i, n in enumerate(nodes) if n.labels.get(LABEL_PROVISIONER))
    # ... and the node that takes the pods of candidate `c` is tainted: they must go elsewhere
    takers = []
    for c in (i for i in range(len(nodes)) if i != mover and bound[i] and nodes[i].labels.get(LABEL_PROVISIONER)):
        before = O.solve(W.whatif(its, prov, nodes, bound, [c], cps))
        takers = [i for i, n in enumerate(nodes) if before.existing.get(n.name) and i != mover]
        if takers:
            break
    assert takers, "the shape must let an existing node take a candidate's pods"
    c_name, taker_name = nodes[c].name, nodes[takers[0]].name
    last = [("node=", W.updated_node(rs, nodes[mover], "zone")), ("node=", dataclasses.replace(nodes[takers[0]], taints=nodes[takers[0]].taints + [W.UPDATE_TAINTS[0]]))]
    info = parsed.apply_block(last)
    assert info["applied"] == 2
    all_events += last
    nodes, bound, slot_of = after(nodes0, bound0, all_events)
    fresh_snap, fresh_pn = W.snapshot_problem(its, prov, nodes, bound, cps)
    fresh = S.ParsedProblem(fresh_snap)
    owned = [i for i, n in enumerate(nodes) if n.labels.get(LABEL_PROVISIONER)]      # (candidates are nodes a provisioner owns: helpers.go:171-230)
    c = [n.name for n in nodes].index(c_name)
    sets = [[c]] + [[int(x) for x in rs.choice(owned, size=int(rs.choice([1, 1, 2, 4])), replace=False)] for _ in range(15)]
    got_f = S.open_whatifs(parsed, None, [[slot_of[j] for j in cs] for cs in sets], derive=True, volumes=volumes)
    want_f = S.open_whatifs(fresh, fresh_pn, sets, derive=True, volumes=volumes)
    try:
        got, _, _ = S.solve_batch(got_f)
        want, _, _ = S.solve_batch(want_f)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g.canonical() == w.canonical() and g.reasons == w.reasons, (seed, i, sets[i])
        for i in range(0, len(sets), 5):
            ref = O.solve(W.whatif(its, prov, nodes, bound, sets[i], cps))
            assert got[i].canonical() == ref.canonical(), (seed, i, sets[i])
        assert not got[0].existing.get(taker_name) and got[0].canonical() != before.canonical()      # the taint was seen
    finally:
        for f in got_f + want_f:
            f.close()
        parsed.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 2 + 3. commands unblock, candidates
def unblock_shape():
    """24 owned nodes at 30-70 % (their pods fit elsewhere: singletons delete), node 5 uninitialised (label "false"), and one more node no provisioner owns that is
    uninitialised too -- so both values of the label are in the cluster before and after the update, and the unowned node blocks nothing (helpers.go:102-111 walks
    the owned existing nodes).  -> (Snapshot before, Snapshot after, the updated node, 16 singleton candidate sets)"""
    its, prov, nodes, bound = W.cluster_snapshot(24, 8, 612)
    nodes[5].labels[INIT] = "false"
    other = W.fresh_node(its, "unowned-uninitialised", np.random.RandomState(1))
    del other.labels[LABEL_PROVISIONER]
    other.labels[INIT] = "false"
    nodes, bound = nodes + [other], bound + [[]]
    assert sum(len(b) for b in bound) <= 300
    before = C.Snapshot(its, prov, nodes, bound)
    ready = dataclasses.replace(nodes[5], labels=dict(nodes[5].labels, **{INIT: "true"}))
    after = C.Snapshot(its, prov, [ready if i == 5 else n for i, n in enumerate(nodes)], bound)
    sets = [[i] for i in range(24) if i != 5][:16]
    return before, after, ready, sets


def test_the_unblock_shape_on_the_reference():
    """No device: the reference restatement gives no delete / replace while node 5 is uninitialised and at least one once it is."""
    before, after, _, sets = unblock_shape()
    assert all(CR.compute_consolidation(before, cs)[0] == "do-nothing" for cs in sets)
    assert any(CR.compute_consolidation(after, cs)[0] in ("delete", "replace") for cs in sets)


def command_rows(parsed, pod_node, snap, sets, leaving):
    words = C._words(snap)
    rows, _ = S.consolidation_commands(parsed, pod_node, sets, words, deleting=leaving)
    return rows, [plain(list(C._command_of_row(snap, parsed, rows[i], words, cs).canonical())) for i, cs in enumerate(sets)]


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["text", "block"])
def test_commands_unblock_and_the_candidate_reason_clears(door):
    before, after, ready, sets = unblock_shape()
    info = C.CandidateInfo(node_age_seconds=[0.0] * len(before.nodes))
    parsed, pn, leaving = C._command_snapshot(before)
    fresh_b, pn_b, _ = C._command_snapshot(before)
    fresh_a, pn_a, _ = C._command_snapshot(after)
    try:
        rows0, cmds0 = command_rows(parsed, pn, before, sets, leaving)
        assert rows0.tobytes() == command_rows(fresh_b, pn_b, before, sets, leaving)[0].tobytes()
        assert all(int(r[S.KS_CMD_DECISION]) & 0xFF == S.KS_CMD_DO_NOTHING for r in rows0)      # blocked: helpers.go:102-113
        cand0, _ = C._candidates_call(S, parsed, pn, before, info)
        assert int(cand0["why"][5]) == WHY_UNINITIALISED and 5 not in cand0["order"]
        got = apply_through(parsed, door, [("node=", ready)], pn)
        assert got["applied"] == 1 and got["continued"] and got["nodes"] == len(before.nodes)
        rows1, cmds1 = command_rows(parsed, None, after, sets, leaving)
        assert rows1.tobytes() == command_rows(fresh_a, pn_a, after, sets, leaving)[0].tobytes()
        want = [plain(list(CR.canonical(CR.compute_consolidation(after, cs)))) for cs in sets]
        assert cmds1 == want
        assert any(c[0] in ("delete", "replace") for c in cmds1) and all(c[0] == "do-nothing" for c in cmds0)
        cand1, _ = C._candidates_call(S, parsed, None, after, info)
        cand_fresh, _ = C._candidates_call(S, fresh_a, pn_a, after, info)
        assert int(cand1["why"][5]) == 0 and 5 in cand1["order"]
        assert list(cand1["order"]) == list(cand_fresh["order"]) and [int(x) for x in cand1["why"]] == [int(x) for x in cand_fresh["why"]]
    finally:
        parsed.close(); fresh_b.close(); fresh_a.close()


# ---------------------------------------------------------------------------------------------------------------- 4. validation
def validation_shape():
    """suite_test.go's "can delete nodes": n1's pod fits n2, the only other node.  NOW n2 carries a taint the pod does not tolerate."""
    then, cands, _ = TC.scenarios()["can_delete_nodes"]
    tainted = dataclasses.replace(then.nodes[1], taints=[W.UPDATE_TAINTS[1]])
    now = C.Snapshot(then.instance_types, then.provisioner, [then.nodes[0], tainted], then.bound)
    return then, now, tainted, cands


def test_the_validation_shape_on_the_reference():
    then, now, _, cands = validation_shape()
    cmd = CR.compute_consolidation(then, cands)
    assert cmd[0] == "delete"
    assert CR.validate_command(then, cmd[0], cmd[1], [], [0, 1]) is True
    assert CR.validate_command(now, cmd[0], cmd[1], [], [0, 1]) is False


def validation(parsed, pod_node, snap, cmd, leaving):
    info = C.CandidateInfo(node_age_seconds=[0.0] * len(snap.nodes))
    got, nf = C._candidates_call(S, parsed, pod_node, snap, info)
    node_sets, expect, type_sets = C._command_inputs_now(snap, [cmd])
    words = C._words(snap)
    rows, _ = S.validate_commands(parsed, pod_node, node_sets, expect, type_sets, got["why"], nf, words, deleting=leaving)
    return rows, S.decode_validation_row(rows[0], words)


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["text", "block"])
def test_a_delete_stops_being_valid_once_the_only_node_with_room_is_tainted(door):
    then, now, tainted, cands = validation_shape()
    parsed, pn, leaving = C._command_snapshot(then)
    fresh, pn_f, _ = C._command_snapshot(now)
    try:
        words = C._words(then)
        rows, _ = S.consolidation_commands(parsed, pn, [cands], words, deleting=leaving)
        cmd = C._command_of_row(then, parsed, rows[0], words, cands)
        assert cmd.action == C.ACTION_DELETE
        _, d0 = validation(parsed, pn, then, cmd, leaving)
        assert d0["valid"] is True
        got = apply_through(parsed, door, [("node=", tainted)], pn)
        assert got["applied"] == 1
        rows1, d1 = validation(parsed, None, now, cmd, leaving)
        rows_f, d_f = validation(fresh, pn_f, now, cmd, leaving)
        assert rows1.tobytes() == rows_f.tobytes()
        assert d1["valid"] is False and (d1["valid"], d1["why"]) == (d_f["valid"], d_f["why"]) != (d0["valid"], d0["why"])
        assert d1["valid"] == CR.validate_command(now, cmd.action, cmd.nodes_to_remove, [], [0, 1])
    finally:
        parsed.close(); fresh.close()
