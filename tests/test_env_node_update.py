"""The fifth event of both doors: NODE= (kshost.h KSH_EVENT_NODE_UPDATE) -- state.Cluster.UpdateNode for a node that is in state already (reference
pkg/controllers/state/cluster.go:151-166, newStateFromNode :227-255: "called for every node reconciliation").  The node object is replaced in its slot; its pods and
bindings stay; labels, taints, available, capacity, daemonset requests, host ports, volume limits and volumes are the record's, taken as given.

CPU half.  The checks are equalities -- two roads to the same flattening -- not tolerances:
  1. a flattening CONTINUED over 1 000 events, a quarter of them NODE=, equals one from scratch after every batch, and a fresh ingest of the model's cluster
     (`workloads.cluster_after`) while no tombstone is in the way; kinds plain / topology / volumes, with and without KSH_ACTIVE_RESOURCES, volumes also under
     KSH_DERIVE_VOLUMES; `ksh_check_whatif_derivation` holds at the end;
  2. every field of the record crosses, through each door;
  3. both doors agree;
  4. the continuation happens where the universes do not move, and does not where they do;
  5. what the door refuses;
  6. a stream without NODE= flattens to what the full run gives.
The GPU half is tests/test_env_node_update_gpu.py."""
import dataclasses

import numpy as np
import pytest

from karpenter_core_amd import model as M
from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import HostPort, Taint, Volume
from test_env_apply_block import (events_for, fingerprints, fresh_in_library_order, make_cluster, raw_apply_block, rich_snapshot, same_info)
from test_whatif_volumes import cluster_after_with_volumes

FLAGS = {"plain": dict(), "active": dict(active_resources=True), "derive_volumes": dict(volumes=True)}
VARIANTS = [(k, f) for k in ("plain", "topology", "volumes") for f in ("plain", "active")] + [("volumes", "derive_volumes")]


def model_after(kind):
    return cluster_after_with_volumes if kind == "volumes" else W.cluster_after


def joining_node(kind):
    def make(its, name, rs):
        n = W.fresh_node(its, name, rs)
        if kind == "volumes":
            n.volume_limits = {W.EBS_DRIVER: int(rs.choice([2, 3, 25]))}
        return n
    return make


def stream(kind, rs, its, nodes, bound, n, tag, make_pod, removes=True, kinds=None):
    """`workloads.random_events_with_updates` for a cluster of a kind: a CSINode limit arrives or changes only in the cluster that has CSI drivers (a limit on any
    node makes the what-ifs of a snapshot underivable without KSH_DERIVE_VOLUMES)."""
    kinds = kinds or tuple(k for k in W.UPDATE_KINDS if kind == "volumes" or k != "volume_limits")
    return W.random_events_with_updates(rs, its, nodes, bound, n, tag, removes=removes, make_pod=make_pod, after=model_after(kind), new_node=joining_node(kind), kinds=kinds)


def apply_through(parsed, door, events, pod_node=None):
    return parsed.apply(events, pod_node) if door == "text" else parsed.apply_block(events, pod_node)


# ---------------------------------------------------------------------------------------------------------------- 1. continued equals cold
@pytest.mark.parametrize("kind,flag", VARIANTS)
def test_continued_equals_cold_over_a_thousand_events(kind, flag):
    fl = FLAGS[flag]
    its, prov, nodes0, bound0, cps, make = make_cluster(kind, 40, 10, 900 + 7 * VARIANTS.index((kind, flag)))
    snap, pn = W.snapshot_problem(its, prov, nodes0, bound0, cps)
    parsed = S.ParsedProblem(snap)
    assert parsed.snapshot_fingerprint(pn, **fl) == parsed.snapshot_fingerprint(pn, cold=True, **fl)
    rs = np.random.RandomState(31 + VARIANTS.index((kind, flag)))
    nodes, bound, all_events, done, call, updates, continued, seen = nodes0, bound0, [], 0, 0, 0, 0, set()
    while done < 1000:
        adds_only = call < 4
        events, nodes, bound = stream(kind, rs, its, nodes, bound, 25, f"c{call}", make, removes=not adds_only)
        all_events += events
        updates += sum(e[0] == "node=" for e in events)
        info = apply_through(parsed, "block" if call % 2 else "text", events, pn if call == 0 else None)
        assert info["applied"] == len(events)
        continued += info["continued"]
        warm, cold = parsed.snapshot_fingerprint(**fl), parsed.snapshot_fingerprint(cold=True, **fl)
        assert warm == cold, (call, [e[:1] for e in events])
        assert warm not in seen      # (every batch moved the flattening)
        seen.add(warm)
        if adds_only:      # no tombstone yet: the library's slots are the model's indices, its pods the original ones then the bound ones in event order
            nodes_now, _, slot = model_after(kind)(nodes0, bound0, all_events)
            assert slot == list(range(len(nodes_now)))
            fresh, fresh_pn = fresh_in_library_order(snap, nodes0, bound0, nodes_now, all_events, cps)
            assert list(parsed.bindings()[0]) == fresh_pn
            fp = S.ParsedProblem(fresh)
            assert warm == fp.snapshot_fingerprint(fresh_pn, **fl), call
            fp.close()
        call += 1
        done += len(events)
    assert 180 <= updates <= 320 and continued >= 1
    bind, slots = parsed.bindings()
    live = [i for i in range(slots) if (bind == i).any()]
    derive = dict(fl, volumes=kind == "volumes")      # (what-ifs over volume limits are derived under KSH_DERIVE_VOLUMES only)
    for cs in ([live[0]], live[1:4], live[::5]):
        S.check_whatif_derivation(parsed, None, cs, **derive)
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 2. every field crosses
FIELD_UPDATES = {
    "labels": lambda n: dict(n.labels, **{M.LABEL_ZONE: [z for z in W.ZONES if z != n.labels[M.LABEL_ZONE]][0]}),
    "taints": lambda n: n.taints + [Taint("dedicated", "storage", "NoSchedule")],
    "available": lambda n: dict(n.available, cpu="250m"),
    "capacity": lambda n: dict(n.capacity, cpu=str(int(n.capacity["cpu"]) + 3)),
    "daemonset_requests": lambda n: {"cpu": "150m", "memory": "1Gi"},
    "host_ports": lambda n: n.host_ports + [HostPort(9100, "TCP", "0.0.0.0")],
    "volume_limits": lambda n: dict(n.volume_limits, **{W.EBS_DRIVER: n.volume_limits[W.EBS_DRIVER] + 1}),
    "volumes": lambda n: n.volumes + [Volume(W.EBS_DRIVER, "default/listed-by-the-node")],
}


@pytest.mark.parametrize("door", ["text", "block"])
@pytest.mark.parametrize("field", sorted(FIELD_UPDATES))
def test_every_field_crosses(field, door):
    """Exactly one field of the record differs from what the slot held: every flattening of the snapshot (flags 0 and KSH_DERIVE_VOLUMES, continued and from
    scratch) equals that of a snapshot ingested with the updated node in place, and differs from the one before the update.  The snapshot has a provisioner with
    limits (capacity counts), a daemonset (daemonset requests count) and volume limits, so that each field reaches the flat problem."""
    snap, pn, nodes0, bound0 = rich_snapshot()
    assert set(FIELD_UPDATES) == {f.name for f in dataclasses.fields(nodes0[2])} - {"name", "in_state"}
    target = 2
    new = dataclasses.replace(snap.nodes[target], **{field: FIELD_UPDATES[field](snap.nodes[target])})
    fresh = S.ParsedProblem(dataclasses.replace(snap, nodes=[new if i == target else n for i, n in enumerate(snap.nodes)]))
    for volumes in (False, True):
        parsed = S.ParsedProblem(snap)
        before = parsed.snapshot_fingerprint(pn, volumes=volumes)      # (flattened before the event: the event continues this flattening)
        info = apply_through(parsed, door, [("node=", new)], pn)
        assert info["applied"] == 1 and info["nodes"] == len(snap.nodes) and info["pods"] == len(pn)
        assert list(parsed.bindings()[0]) == list(pn)
        got = parsed.snapshot_fingerprint(volumes=volumes)
        assert got == parsed.snapshot_fingerprint(cold=True, volumes=volumes) == fresh.snapshot_fingerprint(pn, volumes=volumes)
        assert got != before, f"{field} does not reach the flattening (volumes={volumes})"
        parsed.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 3. both doors agree
@pytest.mark.parametrize("kind", ["plain", "topology", "volumes"])
def test_both_doors_agree(kind):
    its, prov, nodes, bound, cps, make = make_cluster(kind, 32, 8, 640 + len(kind))
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, cps)
    text, block = S.ParsedProblem(snap), S.ParsedProblem(snap)
    for p in (text, block):
        p.snapshot_fingerprint(pn, volumes=kind == "volumes")
    rs = np.random.RandomState(3)
    for call in range(8):
        events, nodes, bound = stream(kind, rs, its, nodes, bound, 12, f"d{call}", make, removes=call >= 2)
        it, ib = text.apply(events, pn if call == 0 else None), block.apply_block(events, pn if call == 0 else None)
        assert ib["applied"] == len(events) and same_info(it, ib), (call, it, ib)
        ft, fb = fingerprints(text, kind), fingerprints(block, kind)
        assert ft == fb and fb[0] == fb[1] and fb[-2] == fb[-1], call
        assert list(text.bindings()[0]) == list(block.bindings()[0])
    text.close(); block.close()


# ---------------------------------------------------------------------------------------------------------------- 4. the continuation happens
DONGLE = "example.com/dongle"


def continuation_snapshot():
    """32 nodes; node 1 is uninitialised (the label's two values are both in the cluster), node 2 carries UPDATE_TAINTS[0] (the taint is in the known set) and every
    node lists a resource nothing requests or limits (inert under KSH_ACTIVE_RESOURCES); the provisioner has a limit."""
    its, prov, nodes, bound = W.cluster_snapshot(32, 8, 77)
    prov = dataclasses.replace(prov, limits={"cpu": "100000"})      # (a node's capacity counts against it)
    nodes[1].labels["karpenter.sh/initialized"] = "false"
    nodes[2].taints = [W.UPDATE_TAINTS[0]]
    for n in nodes:
        n.capacity[DONGLE] = "2"
        n.available[DONGLE] = "2"
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    return snap, pn, nodes


def _updates():
    flip = lambda n: dataclasses.replace(n, labels=dict(n.labels, **{"karpenter.sh/initialized": "false" if n.labels["karpenter.sh/initialized"] == "true" else "true"}))
    return {
        "initialised flip": (1, flip, True, True),
        "initialised flip the other way": (5, flip, True, True),
        "taint added from the known set": (7, lambda n: dataclasses.replace(n, taints=[W.UPDATE_TAINTS[0]]), True, True),
        "taint removed": (2, lambda n: dataclasses.replace(n, taints=[]), True, True),
        "available changed": (3, lambda n: dataclasses.replace(n, available=dict(n.available, cpu="123m")), True, True),
        "capacity changed": (3, lambda n: dataclasses.replace(n, capacity=dict(n.capacity, cpu="7")), True, True),
        "a new label value": (4, lambda n: dataclasses.replace(n, labels=dict(n.labels, **{M.LABEL_ZONE: "test-zone-9"})), False, False),
        "a new taint": (4, lambda n: dataclasses.replace(n, taints=[Taint("never", "seen", "NoSchedule")]), False, False),
        "a new resource name": (4, lambda n: dataclasses.replace(n, available=dict(n.available, **{"example.com/other": "1"})), False, True),      # (inert under the flag)
        "daemonset requests name an inert resource": (6, lambda n: dataclasses.replace(n, daemonset_requests={DONGLE: "1"}), True, False),
    }


@pytest.mark.parametrize("active", [False, True])
@pytest.mark.parametrize("door", ["text", "block"])
@pytest.mark.parametrize("case", sorted(_updates()))
def test_continuation_happens(case, door, active):
    """info[3]: 1 for the updates that leave the universes alone, 0 for those that move them -- and the same bytes either way."""
    slot, change, plain_continues, active_continues = _updates()[case]
    snap, pn, nodes = continuation_snapshot()
    parsed = S.ParsedProblem(snap)
    before = parsed.snapshot_fingerprint(pn, active_resources=active)
    new = change(nodes[slot])
    info = apply_through(parsed, door, [("node=", new)], pn)
    assert info["continued"] == (active_continues if active else plain_continues), case
    got = parsed.snapshot_fingerprint(active_resources=active)
    fresh = S.ParsedProblem(dataclasses.replace(snap, nodes=[new if i == slot else n for i, n in enumerate(snap.nodes)]))
    assert got == parsed.snapshot_fingerprint(cold=True, active_resources=active) == fresh.snapshot_fingerprint(pn, active_resources=active)
    # what the flattening does not read: the initialised label (the command and candidate tables do); a resource name that stays inert; daemonset requests where
    # no daemonset runs (they are taken off nothing) -- under the flag the name they bring is one more resource of the flat problem
    unread = "initialised" in case or (active and case == "a new resource name") or (not active and case == "daemonset requests name an inert resource")
    assert (got == before) == unread
    parsed.close(); fresh.close()


def test_the_last_use_of_a_label_value_leaves_with_the_update():
    """A value only node 4 carried: once the update takes it away the universe of the key shrinks, so the flattening starts over (info[3] = 0) -- same bytes."""
    its, prov, nodes, bound = W.cluster_snapshot(16, 8, 78)
    pod = dataclasses.replace(bound[0][0], node_selector={"team": "a"})      # (the key is referenced: its values are a universe)
    bound[0][0] = pod
    nodes[4].labels["team"] = "only-here"
    nodes[5].labels["team"] = "a"
    nodes[6].labels["team"] = "a"
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    parsed.snapshot_fingerprint(pn)
    shared = dataclasses.replace(nodes[5], labels=dict(nodes[5].labels, team="b-new"))
    assert not parsed.apply([("node=", shared)], pn)["continued"]                       # a new value
    back = dataclasses.replace(nodes[5], labels=dict(nodes[5].labels))
    assert not parsed.apply([("node=", back)])["continued"]                             # its last use goes
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    other = dataclasses.replace(nodes[6], labels={k: v for k, v in nodes[6].labels.items() if k != "team"})
    assert parsed.apply([("node=", other)])["continued"]                                # "a" stays: node 5 and the pod's selector hold it
    gone = dataclasses.replace(nodes[4], labels={k: v for k, v in nodes[4].labels.items() if k != "team"})
    assert not parsed.apply_block([("node=", gone)])["continued"]                       # the last use of "only-here"
    now = [back if i == 5 else other if i == 6 else gone if i == 4 else n for i, n in enumerate(snap.nodes)]
    fresh = S.ParsedProblem(dataclasses.replace(snap, nodes=now))
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True) == fresh.snapshot_fingerprint(pn)
    parsed.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("door", ["text", "block"])
def test_unknown_and_tombstoned_names_are_refused(door):
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed, two = S.ParsedProblem(snap), S.ParsedProblem(snap)
    for p in (parsed, two):
        p.snapshot_fingerprint(pn)
    rs = np.random.RandomState(1)
    good = [("node=", W.updated_node(rs, nodes[1], "zone")), ("bind", nodes[1].name, W.generic_pod(rs, "late"))]
    with pytest.raises(S.KSolveError) as ei:
        apply_through(parsed, door, good + [("node=", dataclasses.replace(nodes[2], name="nobody")), ("node-", nodes[0].name)], pn)
    assert "event 2: NODE=: no state node named nobody (the events before it were applied)" in str(ei.value) and ei.value.code == S.KS_ERR_INVALID
    if door == "block":
        assert ei.value.info["applied"] == 2 and ei.value.info["nodes"] == 8 and ei.value.info["pods"] == len(pn) + 1
    assert apply_through(two, door, good, pn)["applied"] == 2
    assert parsed.snapshot_fingerprint() == two.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    assert list(parsed.bindings()[0]) == list(two.bindings()[0])
    # a node that left is not live: its name is refused until a NODE+ brings it back
    with pytest.raises(S.KSolveError, match=f"event 1: NODE=: no state node named {nodes[3].name} "):
        apply_through(parsed, door, [("node-", nodes[3].name), ("node=", nodes[3])])
    assert parsed.bindings()[1] == 8
    parsed.close(); two.close()


@pytest.mark.parametrize("first_call", [False, True])
def test_a_malformed_update_applies_nothing(first_call):
    """The binary door decodes the whole block first: a NODE= record cut short, or one that names a string the table does not have, is KS_ERR_INVALID with the event's
    index, info all zero, and nothing applied -- not the good event in front of it, not the hand-over of the bindings on a first call."""
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    rs = np.random.RandomState(0)
    if not first_call:
        assert parsed.apply_block([("bind", nodes[0].name, W.generic_pod(rs, "early"))], pn)["applied"] == 1
    fpn = pn if first_call else None
    before = parsed.snapshot_fingerprint(fpn), parsed.snapshot_fingerprint(fpn, cold=True)
    bind_before = None if first_call else list(parsed.bindings()[0])
    good = M.delta_to_block([("unbind", bound[2][0].uid), ("node=", W.updated_node(rs, nodes[1], "taint"))])
    assert int(good["words"][0]) == M.EVENT_UNBIND and int(good["words"][2]) == M.EVENT_NODE_UPDATE == 5

    def variant(**kw):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        b.update(kw)
        return b
    w = good["words"].copy(); w[3] = good["n_strings"] + 3      # the record's first word: the node's name
    bad = [("cut short", variant(n_words=good["n_words"] - 1), "event 1"), ("cut inside the labels", variant(n_words=8), "event 1"),
           ("string id out of range", variant(words=w), "event 1: pod block: string id out of range")]
    for name, blk, needle in bad:
        rc, msg, info = raw_apply_block(parsed, blk, pod_node=fpn)
        assert rc == S.KS_ERR_INVALID and needle in msg and "delta block" in msg, (name, rc, msg)
        assert info == [0, 0, 0, 0], (name, info)
        assert (parsed.snapshot_fingerprint(fpn), parsed.snapshot_fingerprint(fpn, cold=True)) == before, name
        if first_call:
            with pytest.raises(S.KSolveError, match="no ksh_env_apply yet"):
                parsed.bindings()
        else:
            assert list(parsed.bindings()[0]) == bind_before, name
    rc, msg, info = raw_apply_block(parsed, good, pod_node=fpn)
    assert rc == S.KS_OK and info[0] == 2, msg
    assert parsed.snapshot_fingerprint() != before[0]
    parsed.close()


@pytest.mark.parametrize("door", ["text", "block"])
def test_update_then_remove_then_add_takes_a_new_slot(door):
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    parsed.snapshot_fingerprint(pn)
    rs = np.random.RandomState(2)
    upd = W.updated_node(rs, nodes[3], "taint")
    again = dataclasses.replace(nodes[3], available=dict(nodes[3].available, cpu="1"))
    events = [("node=", upd), ("node-", nodes[3].name), ("node+", again), ("bind", nodes[3].name, W.generic_pod(rs, "back")), ("node=", W.updated_node(rs, again, "zone"))]
    info = apply_through(parsed, door, events, pn)
    assert info["applied"] == 5 and info["nodes"] == 9
    bind, slots = parsed.bindings()
    assert slots == 9 and bind[-1] == 8 and not (bind == 3).any()
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 6. no drift for old streams
@pytest.mark.parametrize("kind", ["plain", "topology", "volumes"])
def test_a_stream_without_updates_flattens_as_the_full_run_does(kind):
    """`test_env_apply_block.test_same_flattening_as_the_text_door`'s stream (seed 1): no NODE= in it.  After every call the continued flattening is the full run's
    over the same objects, and -- while the events only add -- that of a snapshot ingested afresh, which no event code has touched."""
    seed = 1
    its, prov, nodes0, bound0, cps, make = make_cluster(kind, 40, 8, 400 + 10 * seed + ["plain", "topology", "volumes"].index(kind))
    snap, pn = W.snapshot_problem(its, prov, nodes0, bound0, cps)
    parsed = S.ParsedProblem(snap)
    parsed.snapshot_fingerprint(pn, volumes=kind == "volumes")
    rs = np.random.RandomState(seed)
    nodes, bound, all_events, continued = nodes0, bound0, [], 0
    for call in range(10):
        adds_only = call < 4
        events, nodes, bound = events_for(kind, rs, its, nodes, bound, int(rs.randint(1, 7)), f"s{seed}c{call}", make, removes=not adds_only)
        assert all(e[0] != "node=" for e in events)
        all_events += events
        continued += apply_through(parsed, "block" if call % 2 else "text", events, pn if call == 0 else None)["continued"]
        f = fingerprints(parsed, kind)
        assert f[0] == f[1] and f[-2] == f[-1], call
        if adds_only:
            nodes_now, _, _ = model_after(kind)(nodes0, bound0, all_events)
            fresh, fresh_pn = fresh_in_library_order(snap, nodes0, bound0, nodes_now, all_events, cps)
            fp = S.ParsedProblem(fresh)
            assert f[1] == fp.snapshot_fingerprint(fresh_pn, cold=True), call
            fp.close()
    assert continued >= 1
    parsed.close()
