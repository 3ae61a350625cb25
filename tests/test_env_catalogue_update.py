"""The sixth event of both doors: IT= (kshost.h KSH_EVENT_INSTANCE_TYPE_UPDATE) -- the catalogue as cloudProvider.GetInstanceTypes lists it NOW.  The reference asks
the provider on every pass (pkg/controllers/provisioning/provisioner.go:237-296), so an offering that went unavailable, a price that moved and the zone /
capacity-type requirement values that follow availability are always current there.  The event replaces one instance type's record in place: the type keeps its
index, requirements / offerings / capacity / overhead are the record's.

CPU half.  The checks are equalities -- two roads to the same flattening -- not tolerances:
  1. a flattening CONTINUED over ~300 events, a third of them IT=, equals one from scratch after every batch, and a fresh ingest of the model's cluster and
     catalogue while no tombstone is in the way; kinds plain / topology / volumes, with and without KSH_ACTIVE_RESOURCES;
  2. every field of the record crosses, through each door;
  3. the continuation happens where the universes do not move, and does not where they do;
  4. both doors agree;
  5. what the door refuses;
  6. the environment object (`PODS 0`) follows the event;
  7. a handle opened before the event keeps its problem.
The GPU half is tests/test_env_catalogue_update_gpu.py."""
import dataclasses

import numpy as np
import pytest

from karpenter_core_amd import model as M
from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import Expr, Offering, pods_to_blocks
from test_env_apply_block import fingerprints, fresh_in_library_order, make_cluster, raw_apply_block, same_info
from test_env_node_update import apply_through, joining_node, model_after

FLAGS = {"plain": dict(), "active": dict(active_resources=True)}
VARIANTS = [(k, f) for k in ("plain", "topology", "volumes") for f in ("plain", "active")]
KINDS = ("availability", "availability", "price", "price", "pair", "pair", "values", "values", "rare")      # (one change in nine brings or takes something rare)


def stream(kind, rs, its, nodes, bound, n, tag, make_pod, removes=True):
    """`workloads.random_events_with_catalogue` for a cluster of a kind (a CSINode limit arrives or changes only in the cluster that has CSI drivers)."""
    node_kinds = tuple(k for k in W.UPDATE_KINDS if kind == "volumes" or k != "volume_limits")
    return W.random_events_with_catalogue(rs, its, nodes, bound, n, tag, changes=KINDS, kinds=node_kinds, removes=removes, make_pod=make_pod, after=model_after(kind),
                                          new_node=joining_node(kind), share=0.3)


def with_type(snap, new):
    return dataclasses.replace(snap, instance_types=[new if t.name == new.name else t for t in snap.instance_types])


def zone_req(it):
    return [r for r in it.requirements if r.key == M.LABEL_ZONE][0]


# ---------------------------------------------------------------------------------------------------------------- 1. continued equals cold
@pytest.mark.parametrize("kind,flag", VARIANTS)
def test_continued_equals_cold_over_three_hundred_events(kind, flag):
    fl = FLAGS[flag]
    its0, prov, nodes0, bound0, cps, make = make_cluster(kind, 40, 10, 1200 + 7 * VARIANTS.index((kind, flag)))
    snap, pn = W.snapshot_problem(its0, prov, nodes0, bound0, cps)
    parsed = S.ParsedProblem(snap)
    assert parsed.snapshot_fingerprint(pn, **fl) == parsed.snapshot_fingerprint(pn, cold=True, **fl)
    rs = np.random.RandomState(61 + VARIANTS.index((kind, flag)))
    its, nodes, bound, all_events, done, call, changes, continued = its0, nodes0, bound0, [], 0, 0, 0, 0
    derive = dict(fl, volumes=kind == "volumes")      # (what-ifs over volume limits are derived under KSH_DERIVE_VOLUMES only)
    while done < 300:
        adds_only = call < 4
        events, its, nodes, bound = stream(kind, rs, its, nodes, bound, 15, f"c{call}", make, removes=not adds_only)
        all_events += events
        changes += sum(e[0] == "IT=" for e in events)
        info = apply_through(parsed, "block" if call % 2 else "text", events, pn if call == 0 else None)
        assert info["applied"] == len(events)
        continued += info["continued"]
        warm, cold = parsed.snapshot_fingerprint(**fl), parsed.snapshot_fingerprint(cold=True, **fl)
        assert warm == cold, (call, [e[:1] for e in events])
        if adds_only:      # no tombstone yet: the library's slots are the model's indices, its pods the original ones then the bound ones in event order
            nodes_now, _, slot = model_after(kind)(nodes0, bound0, all_events)
            assert slot == list(range(len(nodes_now)))
            fresh, fresh_pn = fresh_in_library_order(snap, nodes0, bound0, nodes_now, all_events, cps)
            assert [t.name for t in its] == [t.name for t in its0] and its == W.catalogue_after(its0, all_events)
            fp = S.ParsedProblem(dataclasses.replace(fresh, instance_types=its))
            assert warm == fp.snapshot_fingerprint(fresh_pn, **fl), call
            fp.close()
        if call % 6 == 5:
            bind, slots = parsed.bindings()
            live = [i for i in range(slots) if (bind == i).any()]
            for cs in ([live[0]], live[1:4], live[::5]):
                S.check_whatif_derivation(parsed, None, cs, **derive)
        call += 1
        done += len(events)
    assert 60 <= changes <= 120 and 1 <= continued < call      # (both roads were taken)
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 2. every field crosses
def _first_available(it):
    return [i for i, o in enumerate(it.offerings) if o.available][0]


def _offering(it, i, **kw):
    return dataclasses.replace(it, offerings=[dataclasses.replace(o, **kw) if j == i else o for j, o in enumerate(it.offerings)])


FIELD_UPDATES = {
    "requirement values": lambda it: dataclasses.replace(it, requirements=[Expr(M.LABEL_ZONE, "In", r.values[:1]) if r.key == M.LABEL_ZONE else r for r in it.requirements]),
    "availability": lambda it: _offering(it, _first_available(it), available=False),
    "price": lambda it: _offering(it, _first_available(it), price=it.offerings[_first_available(it)].price * 3.0),
    "offered pairs": lambda it: dataclasses.replace(it, offerings=it.offerings[1:]),
    "capacity": lambda it: dataclasses.replace(it, capacity=dict(it.capacity, cpu=str(int(it.capacity["cpu"]) + 1))),
    "overhead": lambda it: dataclasses.replace(it, overhead=dict(it.overhead, cpu="300m")),
}


def field_snapshot():
    """24 nodes over 6 sizes; the provisioner has limits, so that a type's capacity counts (it_cap) beside its allocatable (it_alloc)."""
    its, prov, nodes, bound = W.cluster_snapshot(24, 6, 33)
    prov = dataclasses.replace(prov, limits={"cpu": "100000"})
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    target = [i for i, t in enumerate(its) if len(zone_req(t).values) >= 2 and len(t.offerings) >= 3][0]      # (several zones, several pairs)
    return snap, pn, target


@pytest.mark.parametrize("door", ["text", "block"])
@pytest.mark.parametrize("field", sorted(FIELD_UPDATES))
def test_every_field_crosses(field, door):
    """Exactly one field of the record differs from what the slot held: the flattening (continued and from scratch) equals that of a snapshot ingested with the new
    record in the type's place, differs from the one before the event, and a what-if flattened over it shows the offering arrays of the fresh one."""
    snap, pn, target = field_snapshot()
    old = snap.instance_types[target]
    new = FIELD_UPDATES[field](old)
    assert [f.name for f in dataclasses.fields(old) if getattr(old, f.name) != getattr(new, f.name)] == [{"requirement values": "requirements", "availability": "offerings",
            "price": "offerings", "offered pairs": "offerings"}.get(field, field)]
    fresh = S.ParsedProblem(with_type(snap, new))
    parsed = S.ParsedProblem(snap)
    before = parsed.snapshot_fingerprint(pn)      # (flattened before the event: the event continues this flattening or falls back)
    info = apply_through(parsed, door, [("IT=", new)], pn)
    assert info["applied"] == 1 and info["nodes"] == len(snap.nodes) and info["pods"] == len(pn)
    got = parsed.snapshot_fingerprint()
    assert got == parsed.snapshot_fingerprint(cold=True) == fresh.snapshot_fingerprint(pn)
    assert got != before, f"{field} does not reach the flattening"
    a, b = S.open_whatifs(parsed, None, [[1]], derive=False)[0], S.open_whatifs(fresh, pn, [[1]], derive=False)[0]
    assert a.fingerprint() == b.fingerprint()
    ca, cb = a.catalogue(), b.catalogue()
    for k in ("it_offer", "it_price", "it_price_lo"):      # (the lowest prices are in no fingerprint)
        assert np.array_equal(ca[k], cb[k]), k
    a.close(); b.close(); parsed.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the continuation happens
WIDGET = "example.com/widget"


def continuation_snapshot():
    """32 nodes over 8 sizes.  A pod selects on the operating system, so the key's values are a universe; type 0 alone lists RARE_OS."""
    its, prov, nodes, bound = W.cluster_snapshot(32, 8, 79)
    bound[0][0] = dataclasses.replace(bound[0][0], node_selector={M.LABEL_OS: "linux"})
    its = list(its)
    its[0] = dataclasses.replace(its[0], requirements=[Expr(M.LABEL_OS, "In", sorted(r.values + [W.RARE_OS])) if r.key == M.LABEL_OS else r for r in its[0].requirements])
    prov = dataclasses.replace(prov, limits={"cpu": "100000"})
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    return snap, pn


def _changes():
    """name -> (type index, change, info[3] without the flag, with KSH_ACTIVE_RESOURCES; None: nothing is asserted but the bytes)"""
    def flip(it):
        offs = [dataclasses.replace(o, available=(not o.available if j == 0 else o.available)) for j, o in enumerate(it.offerings)]
        return W.with_offerings(it, offs)

    def drop_zone(it):      # every offering of the first zone goes, with the requirement value (other types offer the zone)
        z = it.offerings[0].zone
        return W.with_offerings(it, [o for o in it.offerings if o.zone != z])

    return {
        "an availability flip": (3, flip, True, True),
        "a price change": (3, lambda it: _offering(it, 0, price=it.offerings[0].price * 1.5), True, True),
        "a zone dropped that other types still offer": (4, drop_zone, True, True),
        "a zone no universe has": (3, lambda it: W.with_offerings(it, it.offerings + [Offering("on-demand", W.RARE_ZONE, 1.0)]), False, False),
        "the last use of a requirement value": (0, lambda it: dataclasses.replace(it, requirements=[Expr(M.LABEL_OS, "In", [v for v in r.values if v != W.RARE_OS])
                                                                                                      if r.key == M.LABEL_OS else r for r in it.requirements]), False, False),
        "a resource name new to the universe": (3, lambda it: dataclasses.replace(it, capacity=dict(it.capacity, **{WIDGET: "4"})), False, None),      # (inert under the flag)
        "a capacity change": (3, lambda it: dataclasses.replace(it, capacity=dict(it.capacity, memory="3Gi")), None, None),
        "an overhead change": (3, lambda it: dataclasses.replace(it, overhead=dict(it.overhead, memory="20Mi")), None, None),
    }


@pytest.mark.parametrize("active", [False, True])
@pytest.mark.parametrize("door", ["text", "block"])
@pytest.mark.parametrize("case", sorted(_changes()))
def test_continuation_happens(case, door, active):
    """info[3]: 1 for the changes that leave the universes alone, 0 for those that move them -- and the same bytes either way."""
    t, change, plain_continues, active_continues = _changes()[case]
    snap, pn = continuation_snapshot()
    assert len(zone_req(snap.instance_types[4]).values) >= 2
    parsed = S.ParsedProblem(snap)
    before = parsed.snapshot_fingerprint(pn, active_resources=active)
    new = change(snap.instance_types[t])
    info = apply_through(parsed, door, [("IT=", new)], pn)
    expect = active_continues if active else plain_continues
    if expect is not None:
        assert info["continued"] == expect, case
    got = parsed.snapshot_fingerprint(active_resources=active)
    fresh = S.ParsedProblem(with_type(snap, new))
    assert got == parsed.snapshot_fingerprint(cold=True, active_resources=active) == fresh.snapshot_fingerprint(pn, active_resources=active)
    assert (got == before) == (active and case == "a resource name new to the universe")      # (a name nothing requests is not stored under the flag)
    parsed.close(); fresh.close()


def test_a_value_only_nodes_still_carry_stays_in_the_universe():
    """Type 0 alone lists an offering in a zone of its own -- unavailable, so the zone is no value of its requirement and no topology domain, but one of the zone
    universe --, and a node carries the zone's label.  When the type no longer lists it the zone stays a value of the universe (the node holds it): continued.
    When the node then moves away the value goes with it: the full run, through NODE=, same bytes."""
    its, prov, nodes, bound = W.cluster_snapshot(12, 4, 81)
    lone = "test-zone-lone"
    its = list(its)
    its[0] = W.with_offerings(its[0], its[0].offerings + [Offering("on-demand", lone, 2.0, available=False)])
    nodes[2].labels[M.LABEL_ZONE] = lone
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    parsed.snapshot_fingerprint(pn)
    gone = W.with_offerings(its[0], its[0].offerings[:-1])
    assert parsed.apply([("IT=", gone)], pn)["continued"]
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    moved = dataclasses.replace(nodes[2], labels=dict(nodes[2].labels, **{M.LABEL_ZONE: W.ZONES[0]}))
    assert not parsed.apply([("node=", moved)])["continued"]      # (the catalogue no longer holds the value: the node's was the last use)
    fresh = S.ParsedProblem(dataclasses.replace(with_type(snap, gone), nodes=[moved if i == 2 else n for i, n in enumerate(snap.nodes)]))
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True) == fresh.snapshot_fingerprint(pn)
    back = W.with_offerings(gone, gone.offerings + [Offering("on-demand", lone, 2.0, available=False)])
    assert not parsed.apply_block([("IT=", back)])["continued"]      # (and now the zone is new to the universe)
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    parsed.close(); fresh.close()


def test_two_changes_to_one_type_in_one_call():
    """The flattening before the call saw the type as it was before the FIRST of them."""
    snap, pn = continuation_snapshot()
    parsed = S.ParsedProblem(snap)
    parsed.snapshot_fingerprint(pn)
    a = _changes()["an availability flip"][1](snap.instance_types[3])
    b = _changes()["a price change"][1](a)
    info = parsed.apply_block([("IT=", a), ("IT=", b), ("IT=", _changes()["a price change"][1](snap.instance_types[5]))], pn)
    assert info["applied"] == 3 and info["continued"]
    fresh = S.ParsedProblem(with_type(with_type(snap, b), _changes()["a price change"][1](snap.instance_types[5])))
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True) == fresh.snapshot_fingerprint(pn)
    parsed.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 4. both doors agree
@pytest.mark.parametrize("kind", ["plain", "topology", "volumes"])
def test_both_doors_agree(kind):
    its, prov, nodes, bound, cps, make = make_cluster(kind, 32, 8, 660 + len(kind))
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, cps)
    text, block = S.ParsedProblem(snap), S.ParsedProblem(snap)
    for p in (text, block):
        p.snapshot_fingerprint(pn, volumes=kind == "volumes")
    rs = np.random.RandomState(5)
    for call in range(8):
        events, its, nodes, bound = stream(kind, rs, its, nodes, bound, 12, f"d{call}", make, removes=call >= 2)
        assert any(e[0] == "IT=" for e in events)
        it, ib = text.apply(events, pn if call == 0 else None), block.apply_block(events, pn if call == 0 else None)
        assert ib["applied"] == len(events) and same_info(it, ib), (call, it, ib)
        ft, fb = fingerprints(text, kind), fingerprints(block, kind)
        assert ft == fb and fb[0] == fb[1] and fb[-2] == fb[-1], call
        assert list(text.bindings()[0]) == list(block.bindings()[0])
    text.close(); block.close()


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("door", ["text", "block"])
def test_an_unknown_type_name_is_refused(door):
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed, two = S.ParsedProblem(snap), S.ParsedProblem(snap)
    for p in (parsed, two):
        p.snapshot_fingerprint(pn)
    rs = np.random.RandomState(1)
    good = [("IT=", W.updated_type(rs, its[1], "price")), ("bind", nodes[1].name, W.generic_pod(rs, "late"))]
    with pytest.raises(S.KSolveError) as ei:
        apply_through(parsed, door, good + [("IT=", dataclasses.replace(its[2], name="nobody")), ("node-", nodes[0].name)], pn)
    assert "event 2: IT=: no instance type named nobody (the events before it were applied)" in str(ei.value) and ei.value.code == S.KS_ERR_INVALID
    if door == "block":
        assert ei.value.info["applied"] == 2 and ei.value.info["nodes"] == 8 and ei.value.info["pods"] == len(pn) + 1
    assert apply_through(two, door, good, pn)["applied"] == 2
    assert parsed.snapshot_fingerprint() == two.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    assert list(parsed.bindings()[0]) == list(two.bindings()[0])
    parsed.close(); two.close()


@pytest.mark.parametrize("door", ["text", "block"])
@pytest.mark.parametrize("what", ["Gt", "hostname"])
def test_a_record_the_ingest_refuses_is_refused(what, door):
    """What ksh_parse + flattening answer with KS_ERR_UNSUPPORTED for an instance type is refused by the event with the same code, and the type stays as it was."""
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    before = parsed.snapshot_fingerprint(pn)
    extra = Expr(fake_integer_key(), "Gt", ["3"]) if what == "Gt" else Expr(M.LABEL_HOSTNAME, "In", ["some-host"])
    bad = dataclasses.replace(its[2], requirements=its[2].requirements + [extra], offerings=[dataclasses.replace(o, price=o.price * 7) for o in its[2].offerings])
    ingest = S.ParsedProblem(with_type(snap, bad))
    with pytest.raises(S.KSolveError) as ei:
        ingest.snapshot_fingerprint(pn)
    assert ei.value.code == S.KS_ERR_UNSUPPORTED
    ingest.close()
    rs = np.random.RandomState(2)
    with pytest.raises(S.KSolveError) as ei:
        apply_through(parsed, door, [("bind", nodes[1].name, W.generic_pod(rs, "late")), ("IT=", bad)], pn)
    assert ei.value.code == S.KS_ERR_UNSUPPORTED and "event 1: IT=: instance type requirement" in str(ei.value)
    if door == "block":
        assert ei.value.info["applied"] == 1
    two = S.ParsedProblem(snap)
    two.snapshot_fingerprint(pn)
    assert two.apply([("bind", nodes[1].name, W.generic_pod(np.random.RandomState(2), "late"))], pn)["applied"] == 1
    assert parsed.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True) == two.snapshot_fingerprint() != before      # (the bind, and nothing of the type)
    parsed.close(); two.close()


def fake_integer_key():
    from karpenter_core_amd import fake
    return fake.LABEL_INTEGER


@pytest.mark.parametrize("first_call", [False, True])
def test_a_malformed_record_applies_nothing(first_call):
    """The binary door decodes the whole block first: an IT= record cut short, or one that names a string the table does not have, is KS_ERR_INVALID with the event's
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
    good = M.delta_to_block([("unbind", bound[2][0].uid), ("IT=", W.updated_type(rs, its[1], "price"))])
    assert int(good["words"][0]) == M.EVENT_UNBIND and int(good["words"][2]) == M.EVENT_INSTANCE_TYPE_UPDATE == 6

    def variant(**kw):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        b.update(kw)
        return b
    w = good["words"].copy(); w[3] = good["n_strings"] + 3      # the record's first word: the type's name
    bad = [("runs past n_words", variant(n_words=good["n_words"] - 1), "event 1"), ("cut inside the requirements", variant(n_words=8), "event 1"),
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


# ---------------------------------------------------------------------------------------------------------------- 6. the environment object
@pytest.mark.parametrize("door", ["text", "block"])
def test_the_environment_follows_the_event(door):
    """`PODS 0`: the environment a provisioning Solve flattens its batches against.  A batch opened after the event equals the same batch over an environment
    ingested with the new record -- the cached flattening of the environment before the event is not used again."""
    its, prov, nodes, bound = W.cluster_snapshot(16, 6, 9)
    rs = np.random.RandomState(4)
    pods = [W.generic_pod(rs, f"pending-{i}") for i in range(60)]
    env_pr = dataclasses.replace(W.snapshot_problem(its, prov, nodes, bound, False)[0], pods=[], simulation_mode=False)
    env = S.ParsedProblem(env_pr)
    batch = S.PodBatch(pods_to_blocks(pods, 2))
    before = S.open_batch(env, batch)      # (the environment's flattening is cached from here on)
    new = W.with_offerings(its[0], [dataclasses.replace(o, available=False) for o in its[0].offerings])      # (the provider no longer lists the type)
    info = apply_through(env, door, [("IT=", new)])
    assert info["applied"] == 1 and info["pods"] == 0
    after = S.open_batch(env, batch)
    fresh_env = S.ParsedProblem(with_type(env_pr, new))
    fresh = S.open_batch(fresh_env, batch)
    assert after.fingerprint() == fresh.fingerprint() != before.fingerprint()
    assert int(after.catalogue()["it_offer"][0]) == 0 != int(before.catalogue()["it_offer"][0])
    for f in (before, after, fresh):
        f.close()
    batch.close(); env.close(); fresh_env.close()


# ---------------------------------------------------------------------------------------------------------------- 7. old handles keep their problem
def test_a_handle_opened_before_the_event_keeps_its_problem():
    snap, pn = continuation_snapshot()
    parsed = S.ParsedProblem(snap)
    old = S.open_whatifs(parsed, pn, [[1]], derive=False)[0]
    fp0, cat0 = old.fingerprint(), old.catalogue()
    t = 3
    new = _changes()["an availability flip"][1](snap.instance_types[t])
    assert parsed.apply([("IT=", new)], pn)["continued"]
    assert old.fingerprint() == fp0
    cat1 = old.catalogue()
    for k in cat0:
        assert np.array_equal(cat0[k], cat1[k]), k
    now = S.open_whatifs(parsed, None, [[1]], derive=False)[0]
    cat2 = now.catalogue()
    assert int(cat2["it_offer"][t]) != int(cat0["it_offer"][t]) and bin(int(cat2["it_offer"][t]) ^ int(cat0["it_offer"][t])).count("1") == 1
    others = [i for i in range(len(snap.instance_types)) if i != t]
    assert np.array_equal(cat2["it_offer"][others], cat0["it_offer"][others])
    old.close(); now.close(); parsed.close()
