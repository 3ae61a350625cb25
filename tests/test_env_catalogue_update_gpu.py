"""IT= (kshost.h KSH_EVENT_INSTANCE_TYPE_UPDATE) seen by the device paths.  The event has no kernel of its own: the kernels read whatever flattening they are given
-- ks_build_type_tables derives the offering pairs of the feasibility grid from it_offer, ks_price_filter / ks_consolidation_commands / ks_launch_pick /
ks_replacement_nodes read it_price and it_price_lo -- so what is checked here is that each of them SEES the event.  Every case is compared three ways: the patched
snapshot, a freshly ingested snapshot of the same cluster with the new records, and the oracle (`oracle` Solve; oracle/consolidation_ref.py for commands):
  1. the grid sees availability: the only type that was offered where the pod must run drops out of the what-if's InstanceTypeOptions and of the command row;
  2. the price stage sees prices: replace <-> "can't replace with a cheaper node", and the launch pick flips when the cheapest offering's price crosses the other's;
  3. the spot rule sees capacity types: a replacement that loses its on-demand offering makes a spot candidate's command "can't replace a spot node with a spot node";
  4. a provisioning Solve over the environment sees a type that has no available offering left: no new node lists it;
  5. the replacement rows of an expired node after a price change are those over the fresh snapshot.
The shapes are checked on the reference restatement first, without a device.  The CPU half is tests/test_env_catalogue_update.py."""
import dataclasses
import json

import numpy as np
import pytest

from karpenter_core_amd import consolidation as C, fake
from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import LABEL_CAPACITY_TYPE, LABEL_ZONE, Expr, Offering, PreferredTerm, pods_to_blocks
from oracle import consolidation_ref as CR
from oracle import oracle_py as O

import test_consolidation as TC
from test_env_apply_block import make_cluster
from test_env_node_update import apply_through

Z1, Z2 = "test-zone-1a", "test-zone-1b"


def plain(x):
    return json.loads(json.dumps(x))


def with_types(snap, *new):
    by = {t.name: t for t in new}
    return dataclasses.replace(snap, instance_types=[by.get(t.name, t) for t in snap.instance_types])


def offer(it, capacity_type, zone, **kw):
    """`it` with one offering changed, its zone / capacity-type requirement values following availability as the providers derive them"""
    return W.with_offerings(it, [dataclasses.replace(o, **kw) if (o.capacity_type, o.zone) == (capacity_type, zone) else o for o in it.offerings])


def commands(parsed, pod_node, snap, sets, leaving):
    words = C._words(snap)
    rows, _ = S.consolidation_commands(parsed, pod_node, sets, words, deleting=leaving)
    return rows, [plain(list(C._command_of_row(snap, parsed, rows[i], words, cs).canonical())) for i, cs in enumerate(sets)]


def reference(snap, sets):
    return [plain(list(CR.canonical(CR.compute_consolidation(snap, cs)))) for cs in sets]


def reason(row):
    return (int(row[S.KS_CMD_DECISION]) & 0xFF, (int(row[S.KS_CMD_DECISION]) >> 8) & 0xFF)


def three_ways(parsed, snap, sets, leaving):
    """The command rows over the patched snapshot; asserted equal, byte for byte, to those over `snap` ingested afresh, and as commands to the oracle's."""
    rows, cmds = commands(parsed, None, snap, sets, leaving)
    fresh, pn_f, _ = C._command_snapshot(snap)
    try:
        assert rows.tobytes() == commands(fresh, pn_f, snap, sets, leaving)[0].tobytes()
    finally:
        fresh.close()
    assert cmds == reference(snap, sets)
    return rows, cmds


def whatif_nodes(parsed, pod_node, snap, cs):
    """The derived what-if of candidate set `cs`, solved on the device: (flat problem, result); the result asserted equal to the oracle's Solve of the same what-if."""
    f = S.open_whatifs(parsed, pod_node, [cs], derive=True)[0]
    res = S.solve_batch([f])[0][0]
    assert res.canonical() == O.solve(W.whatif(snap.instance_types, snap.provisioner, snap.nodes, snap.bound, cs)).canonical()
    return f, res


# ---------------------------------------------------------------------------------------------------------------- 1. the grid sees availability
def availability_shape():
    """One node of an expensive type in zone 1a; its pod selects that zone.  Type A (0.3) is offered in 1a and 1b, type B in 1b only, type C
    (0.6) in both: the one-node replacement is A or C.  Then A's offering in 1a goes unavailable (its zone requirement follows): A is not offered where the pod must run."""
    cur = fake.new_instance_type("current", {"cpu": "8"}, offerings=[Offering("on-demand", Z1, 1.0, False)])
    a = fake.new_instance_type("type-a", {"cpu": "4"}, offerings=[Offering("on-demand", Z1, 0.3), Offering("on-demand", Z2, 0.3)])
    b = fake.new_instance_type("type-b", {"cpu": "4"}, offerings=[Offering("on-demand", Z2, 0.2)])
    c = fake.new_instance_type("type-c", {"cpu": "4"}, offerings=[Offering("on-demand", Z1, 0.6), Offering("on-demand", Z2, 0.6)])
    p = TC.pod("p1")
    p.node_selector = {LABEL_ZONE: Z1}
    before = TC.snapshot([cur, a, b, c], [TC.node("n1", cur, "on-demand", Z1, cpu="8")], [[p]])
    gone = offer(a, "on-demand", Z1, available=False)
    return before, with_types(before, gone), gone


def test_the_availability_shape_on_the_reference():
    before, after, _ = availability_shape()
    assert CR.compute_consolidation(before, [0])[:3] == ("replace", ["n1"], ["type-a", "type-c"])
    assert CR.compute_consolidation(after, [0])[:3] == ("replace", ["n1"], ["type-c"])


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["text", "block"])
def test_the_grid_sees_availability(door):
    before, after, gone = availability_shape()
    parsed, pn, leaving = C._command_snapshot(before)
    try:
        rows0, cmds0 = commands(parsed, pn, before, [[0]], leaving)
        assert cmds0 == reference(before, [[0]]) and cmds0[0][2] == ["type-a", "type-c"]
        f0, res0 = whatif_nodes(parsed, pn, before, [0])
        assert res0.new_nodes[0].instance_types == ["type-a", "type-c"]
        info = apply_through(parsed, door, [("IT=", gone)], pn)
        assert info["applied"] == 1 and info["continued"]
        f1, res1 = whatif_nodes(parsed, None, after, [0])
        assert res1.new_nodes[0].instance_types == ["type-c"]      # A is not offered where the pod must run
        rows1, cmds1 = three_ways(parsed, after, [[0]], leaving)
        assert cmds1[0][0] == "replace" and cmds1[0][2] == ["type-c"]
        assert rows1.tobytes() != rows0.tobytes()      # (a library that ignored the event would give the row it gave before)
        assert int(f0.catalogue()["it_offer"][1]) != int(f1.catalogue()["it_offer"][1])      # the handle opened before keeps its problem
        f0.close(); f1.close()
    finally:
        parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the price stage sees prices
def price_shape():
    """A node of a type at 0.5; two cheaper types X (0.2) and Y (0.25) can take its pod."""
    cur = fake.new_instance_type("current", {"cpu": "8"}, offerings=[Offering("on-demand", Z1, 0.5, False)])
    x = fake.new_instance_type("type-x", {"cpu": "4"}, offerings=[Offering("on-demand", Z1, 0.2)])
    y = fake.new_instance_type("type-y", {"cpu": "4"}, offerings=[Offering("on-demand", Z1, 0.25)])
    snap = TC.snapshot([cur, x, y], [TC.node("n1", cur, "on-demand", Z1, cpu="8")], [[TC.pod("p1")]])
    steps = [("x above y", [offer(x, "on-demand", Z1, price=0.4)], "replace", ["type-x", "type-y"], "type-y"),
             ("both above the candidate", [offer(x, "on-demand", Z1, price=0.7), offer(y, "on-demand", Z1, price=0.7)], "do-nothing", [], "type-x"),
             ("y back below", [y], "replace", ["type-y"], "type-y")]
    return snap, steps


def test_the_price_shape_on_the_reference():
    snap, steps = price_shape()
    assert CR.compute_consolidation(snap, [0])[:3] == ("replace", ["n1"], ["type-x", "type-y"])
    for name, new, action, options, _ in steps:
        snap = with_types(snap, *new)
        cmd = CR.compute_consolidation(snap, [0])
        assert (cmd[0], list(cmd[2]) if cmd[0] == "replace" else []) == (action, options), name


def pick(parsed, pod_node, snap):
    """ks_launch_pick over the what-if's one new node: (type name, price); asserted equal to the reference's pick and to the pick over a fresh snapshot."""
    f, res = whatif_nodes(parsed, pod_node, snap, [0])
    fresh, pn_f, _ = C._command_snapshot(snap)
    g, _ = whatif_nodes(fresh, pn_f, snap, [0])
    try:
        got, got_f = S.launch_pick([f], [0])[0], S.launch_pick([g], [0])[0]
        assert got == got_f
        assert (snap.instance_types[got[0]].name, got[3]) == CR.launch_pick(snap.instance_types, res.new_nodes[0])
        return snap.instance_types[got[0]].name, got[3]
    finally:
        f.close(); g.close(); fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["text", "block"])
def test_the_price_stage_sees_prices(door):
    snap, steps = price_shape()
    parsed, pn, leaving = C._command_snapshot(snap)
    try:
        rows, cmds = commands(parsed, pn, snap, [[0]], leaving)
        assert cmds == reference(snap, [[0]]) and cmds[0][0] == "replace"
        assert pick(parsed, pn, snap) == ("type-x", 0.2)
        first = True
        for name, new, action, options, picked in steps:
            snap = with_types(snap, *new)
            info = apply_through(parsed, door, [("IT=", t) for t in new], pn if first else None)
            first = False
            assert info["applied"] == len(new) and info["continued"], name
            before, cmds_before = rows, cmds
            rows, cmds = three_ways(parsed, snap, [[0]], leaving)
            assert (cmds[0][0], cmds[0][2]) == (action, options), name
            assert (rows.tobytes() != before.tobytes()) == (cmds != cmds_before), name      # (x above y moves the pick alone: both stay cheaper than the candidate)
            if action == "do-nothing":
                assert reason(rows[0]) == (S.KS_CMD_DO_NOTHING, S.KS_CMD_WHY_NOT_CHEAPER)      # "can't replace with a cheaper node"
            assert pick(parsed, None, snap)[0] == picked, name      # (the launch pick reads the lowest prices: it flips when x crosses y)
    finally:
        parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the spot rule sees capacity types
def spot_shape():
    """A spot node at 0.5 whose pod PREFERS on-demand; the replacement type offers on-demand at 0.3 and spot at 0.2.  While the on-demand offering is there the
    preference holds, the new node requires on-demand and the command is replace.  Once it is gone the preference is relaxed (scheduler.go:119-127), the new node
    may be spot, and a spot node is not replaced with a spot node (consolidation.go:250-260)."""
    cur = fake.new_instance_type("current-spot", {"cpu": "8"}, offerings=[Offering("spot", Z1, 0.5, False)])
    rep = fake.new_instance_type("replacement", {"cpu": "4"}, offerings=[Offering("on-demand", Z1, 0.3), Offering("spot", Z1, 0.2)])
    tiny = fake.new_instance_type("tiny-on-demand", {"cpu": "1"}, offerings=[Offering("on-demand", Z1, 0.05)])      # (too small for the pod; keeps on-demand a capacity type of the catalogue)
    p = TC.pod("p1")
    p.preferred_affinity = [PreferredTerm(1, [Expr(LABEL_CAPACITY_TYPE, "In", ["on-demand"])])]
    before = TC.snapshot([cur, rep, tiny], [TC.node("n1", cur, "spot", Z1, cpu="8")], [[p]])
    lost = offer(rep, "on-demand", Z1, available=False)
    return before, with_types(before, lost), lost


def test_the_spot_shape_on_the_reference():
    before, after, _ = spot_shape()
    assert CR.compute_consolidation(before, [0])[:3] == ("replace", ["n1"], ["replacement"])
    assert CR.compute_consolidation(after, [0])[0] == "do-nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("door", ["text", "block"])
def test_the_spot_rule_sees_capacity_types(door):
    before, after, lost = spot_shape()
    parsed, pn, leaving = C._command_snapshot(before)
    try:
        rows0, cmds0 = commands(parsed, pn, before, [[0]], leaving)
        assert cmds0 == reference(before, [[0]]) and cmds0[0][0] == "replace"
        info = apply_through(parsed, door, [("IT=", lost)], pn)
        assert info["applied"] == 1 and info["continued"]
        rows1, cmds1 = three_ways(parsed, after, [[0]], leaving)
        assert cmds1[0][0] == "do-nothing" and reason(rows1[0]) == (S.KS_CMD_DO_NOTHING, S.KS_CMD_WHY_SPOT_TO_SPOT)
        assert int(rows1[0][S.KS_CMD_N_NEW]) == 1 and int(rows1[0][S.KS_CMD_N_UNSCHEDULED]) == 0      # (the pod schedules, on a spot node)
    finally:
        parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 4. a provisioning Solve sees it
@pytest.mark.gpu
@pytest.mark.parametrize("door", ["text", "block"])
def test_a_provisioning_solve_sees_a_type_without_offerings(door):
    its, prov, nodes, bound, _, make = make_cluster("plain", 40, 10, 731, spare_pod_slots=4)      # (full by pod count: the pending pods need new nodes)
    rs = np.random.RandomState(8)
    pods = [make(rs, f"pending-{i:03d}") for i in range(120)]
    pr = dataclasses.replace(W.snapshot_problem(its, prov, nodes, bound, False)[0], pods=pods, simulation_mode=False)
    env = S.ParsedProblem(dataclasses.replace(pr, pods=[]))
    batch = S.PodBatch(pods_to_blocks(pods, 2))
    f0, f1, f2, fresh_env = None, None, None, None
    try:
        f0, _ = S.solve_from_batch(env, batch, 0)
        res0 = f0.result()
        assert res0.canonical() == O.solve(pr).canonical() and res0.new_nodes
        name = res0.new_nodes[0].instance_types[0]
        t = [x.name for x in its].index(name)
        none_left = W.with_offerings(its[t], [dataclasses.replace(o, available=False) for o in its[t].offerings])
        assert apply_through(env, door, [("IT=", none_left)])["applied"] == 1
        after = with_types(pr, none_left)
        f1, _ = S.solve_from_batch(env, batch, 0)
        res1 = f1.result()
        assert all(name not in n.instance_types for n in res1.new_nodes) and res1.new_nodes
        fresh_env = S.ParsedProblem(dataclasses.replace(after, pods=[]))
        f2, _ = S.solve_from_batch(fresh_env, batch, 0)
        assert res1.canonical() == f2.result().canonical() == O.solve(after).canonical()      # placements and options
        assert f1.fingerprint() == f2.fingerprint() != f0.fingerprint()
    finally:
        for f in (f0, f1, f2):
            if f is not None:
                f.close()
        batch.close(); env.close()
        if fresh_env is not None:
            fresh_env.close()


# ---------------------------------------------------------------------------------------------------------------- 5. replacement rows
@pytest.mark.gpu
def test_replacement_rows_after_a_price_change():
    """Expiration's command for the node of `price_shape` (expiration.go:68-113: no price stage; every type that fits is an option) before and after X's price
    moves: head and node rows over the patched snapshot are those over the fresh one, and the options are the reference's."""
    snap, steps = price_shape()
    parsed, pn, leaving = C._command_snapshot(snap)
    words = C._words(snap)
    try:
        S.replacement_commands(parsed, pn, [[0]], words, deleting=leaving)
        snap = with_types(snap, *steps[1][1])
        assert parsed.apply_block([("IT=", t) for t in steps[1][1]], pn)["continued"]
        heads, nodes, total, _ = S.replacement_commands(parsed, None, [[0]], words, deleting=leaving)
        fresh, pn_f, _ = C._command_snapshot(snap)
        heads_f, nodes_f, total_f, _ = S.replacement_commands(fresh, pn_f, [[0]], words, deleting=leaving)
        assert total == total_f == 1 and heads.tobytes() == heads_f.tobytes() and nodes.tobytes() == nodes_f.tobytes()
        action, removed, replacements = CR.replacement_command(snap, [0])
        d = S.decode_replacement_node(parsed, nodes[0], words)
        assert action == "replace" and sorted(snap.instance_types[t].name for t in d["options"]) == sorted(replacements[0][0])
        fresh.close()
    finally:
        parsed.close()
