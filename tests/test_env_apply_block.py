"""The BINARY door for cluster events (kshost.h `ksh_env_apply_block`, `ksh_delta_block`; grammar in karpenter_core_amd/host/kspb.hpp DeltaReader): the events
`ksh_env_apply` takes as KSD1 text -- state.Cluster's UpdateNode / DeleteNode / UpdatePod / DeletePod (reference pkg/controllers/state/cluster.go) -- as one stream of
u32 words over one string table, the form the other two doors (`ksh_pods_ingest`, `ksh_env_ingest`) already have.

The two doors differ in the decoding alone, so the checks are equalities, not tolerances: a snapshot patched through the binary door must be, byte for byte of its
flattening (`ksh_snapshot_fingerprint`, warm and cold, flags 0 and KSH_DERIVE_VOLUMES), binding for binding and `info` word for `info` word, the snapshot patched
through the text door with the same events -- and, while the events only add, the snapshot a caller would have ingested afresh from the cluster as it is now.
CPU half: (1) that, over seeds x {plain, topology, volumes}; (2) a thousand events with the doors alternating call by call; (3) one handmade node and pod that use
every field of the two record grammars; (4) what the door refuses -- a malformed block applies NOTHING; (5) KSH_APPLY_TRACK_CLUSTER_PODS; (6) the door from plain C.
GPU half (`-m gpu`): derived what-ifs over the block-patched snapshot solve like those over a text-patched twin, a fresh snapshot and the oracle."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from karpenter_core_amd import fake, scheduler as S, workloads as W
from karpenter_core_amd import model as M
from karpenter_core_amd.model import (Container, DO_NOT_SCHEDULE, SCHEDULE_ANYWAY, Expr, HostPort, LABEL_HOSTNAME, LABEL_ZONE, LabelSelector, Pod, PodAffinityTerm,
                                      PreferredTerm, StateNode, Taint, Toleration, TopologySpreadConstraint, Volume, WeightedPodAffinityTerm)
from test_env_apply import random_events, spread_pod
from test_whatif_volumes import cluster_after_with_volumes, volume_pod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["plain", "topology", "volumes"]


# ---------------------------------------------------------------------------------------------------------------- snapshots and events of the three kinds
def make_cluster(kind, existing, sizes, seed, **kw):
    """(its, prov, nodes, bound, with_cluster_pods, pod maker) of a kind: plain pods | a third of them with spread terms, the bound pods listed as cluster pods
    (countDomains) | CSI volume limits and claims (`workloads.volume_snapshot`)."""
    if kind == "volumes":
        its, prov, nodes, bound = W.volume_snapshot(existing, sizes, seed, unowned=False, **kw)
        shared = sorted({v.pvc_id for b in bound for p in b for v in p.volumes if "rwx" in v.pvc_id}) or ["default/rwx-0000"]
        return its, prov, nodes, bound, False, (lambda r, u: volume_pod(r, u, shared))
    its, prov, nodes, bound = W.cluster_snapshot(existing, sizes, seed, **kw)
    if kind == "topology":
        rs0 = np.random.RandomState(seed)
        bound = [[spread_pod(rs0, p.uid) if rs0.randint(3) == 0 else p for p in b] for b in bound]
        return its, prov, nodes, bound, True, (lambda r, u: spread_pod(r, u) if r.randint(3) == 0 else W.generic_pod(r, u))
    return its, prov, nodes, bound, False, W.generic_pod


def events_for(kind, rs, its, nodes, bound, n, tag, make_pod, removes=True):
    """`test_env_apply.random_events`; for the volumes kind the nodes that join carry a CSINode limit and every node's volume usage follows its pods."""
    events, nodes2, bound2 = random_events(rs, its, nodes, bound, n, tag, removes=removes, make_pod=make_pod)
    if kind == "volumes":
        for e in events:
            if e[0] == "node+":
                e[1].volume_limits = {W.EBS_DRIVER: int(rs.choice([2, 3, 25]))}
        nodes2, bound2, _ = cluster_after_with_volumes(nodes, bound, events)
    return events, nodes2, bound2


def after(kind, nodes, bound, events):
    return cluster_after_with_volumes(nodes, bound, events) if kind == "volumes" else W.cluster_after(nodes, bound, events)


def fingerprints(parsed, kind):
    """Every flattening the snapshot has: continued and from scratch, and for a snapshot with volumes the one derived volume what-ifs use as well."""
    out = []
    for volumes in ([False, True] if kind == "volumes" else [False]):
        out += [parsed.snapshot_fingerprint(volumes=volumes), parsed.snapshot_fingerprint(cold=True, volumes=volumes)]
    return out


def same_info(a, b):
    return {k: a[k] for k in ("applied", "nodes", "pods", "continued")} == {k: b[k] for k in ("applied", "nodes", "pods", "continued")}


def flat_hashes(parsed, pod_node, sets):
    flats = S.open_whatifs(parsed, pod_node, sets, derive=False)
    out = [f.fingerprint() for f in flats]
    for f in flats:
        f.close()
    return out


def fresh_in_library_order(snap, nodes0, bound0, nodes_now, all_events, with_cluster_pods):
    """The snapshot a caller would list from the cluster as it is now, after events that only ADD, in the library's pod order: the original pods, then the bound
    ones in event order (the comparison tests/test_env_apply.py makes for the text door)."""
    pods, pod_node = [], []
    for i in range(len(nodes0)):
        for p in bound0[i]:
            pods.append(p)
            pod_node.append(i)
    name_to = {n.name: i for i, n in enumerate(nodes_now)}
    for ev in all_events:
        if ev[0] == "bind":
            pods.append(ev[2])
            pod_node.append(name_to[ev[1]])
    cps = [W.ClusterPod(uid=p.uid, namespace=p.namespace, node_name=nodes_now[pod_node[i]].name, labels=p.labels, anti_required=list(p.anti_required))
           for i, p in enumerate(pods)] if with_cluster_pods else []
    return dataclasses.replace(snap, nodes=[dataclasses.replace(n, in_state=True) for n in nodes_now], pods=pods, cluster_pods=cps), pod_node


# ---------------------------------------------------------------------------------------------------------------- 1. the same flattening as the text door
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_same_flattening_as_the_text_door(seed, kind):
    """Two snapshots ingested from the same objects; one hears the events through `apply`, the other through `apply_block`, call by call.  After EVERY call the
    fingerprints (warm, cold; with volumes: both flattenings), the bindings and info[0..3] are equal; while the events only add (the first four calls) both equal
    the snapshot ingested afresh from the patched object list, what-if for what-if."""
    its, prov, nodes0, bound0, cps, make = make_cluster(kind, 40, 8, 400 + 10 * seed + KINDS.index(kind))
    snap, pn = W.snapshot_problem(its, prov, nodes0, bound0, cps)
    text, block = S.ParsedProblem(snap), S.ParsedProblem(snap)
    for p in (text, block):      # (both are flattened before the first event: the events continue that flattening)
        p.snapshot_fingerprint(pn, volumes=kind == "volumes")
    rs = np.random.RandomState(seed)
    nodes, bound, all_events, continued = nodes0, bound0, [], 0
    for call in range(10):
        adds_only = call < 4
        events, nodes, bound = events_for(kind, rs, its, nodes, bound, int(rs.randint(1, 7)), f"s{seed}c{call}", make, removes=not adds_only)
        all_events += events
        it = text.apply(events, pn if call == 0 else None)
        ib = block.apply_block(events, pn if call == 0 else None)
        assert ib["applied"] == len(events) and same_info(it, ib), (call, it, ib)
        continued += ib["continued"]
        ft, fb = fingerprints(text, kind), fingerprints(block, kind)
        assert ft == fb, (call, [e[:2] for e in events])
        assert all(f == fb[0] for f in fb[:2]) and all(f == fb[2] for f in fb[2:4])      # continued == from scratch, per flattening
        (bt, st), (bb, sb) = text.bindings(), block.bindings()
        assert st == sb == ib["nodes"] and list(bt) == list(bb) and len(bb) == ib["pods"]
        if adds_only:
            nodes_now, _, slot = after(kind, nodes0, bound0, all_events)
            assert slot == list(range(len(nodes_now)))
            fresh, fresh_pn = fresh_in_library_order(snap, nodes0, bound0, nodes_now, all_events, cps)
            assert list(bb) == fresh_pn
            fp = S.ParsedProblem(fresh)
            assert block.snapshot_fingerprint() == fp.snapshot_fingerprint(fresh_pn), call
            if kind == "volumes":
                assert block.snapshot_fingerprint(volumes=True) == fp.snapshot_fingerprint(fresh_pn, volumes=True), call
            sets = [[0], [len(nodes_now) - 1], [1, 2, 3], list(range(0, len(nodes_now), 3))]
            assert flat_hashes(block, None, sets) == flat_hashes(fp, fresh_pn, sets) == flat_hashes(text, None, sets), call
            fp.close()
    assert continued >= 1      # (the short road was taken through the new door too; how often depends on which flattening the fingerprints left cached)
    text.close(); block.close()


# ---------------------------------------------------------------------------------------------------------------- 2. a thousand events, the doors alternating
def test_a_thousand_events_through_alternating_doors():
    """Mixed use is legal: text and binary calls on the same snapshot, alternating call by call, 1 000 events (topology terms in the snapshot, binds / unbinds /
    nodes coming and going).  Every hundred events the device derivation's host restatement holds on a sample of candidate sets, the continued flattening equals
    one from scratch, and the snapshot equals a twin that heard everything through the text door."""
    its, prov, nodes, bound, cps, make = make_cluster("topology", 40, 10, 77)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, cps)
    mixed, twin = S.ParsedProblem(snap), S.ParsedProblem(snap)
    mixed.snapshot_fingerprint(pn); twin.snapshot_fingerprint(pn)
    rs = np.random.RandomState(9)
    done, call = 0, 0
    while done < 1000:
        events, nodes, bound = random_events(rs, its, nodes, bound, 25, f"k{done}", make_pod=make)
        first = pn if call == 0 else None
        im = mixed.apply_block(events, first) if call % 2 == 0 else mixed.apply(events, first)
        it = twin.apply(events, first)
        assert im["applied"] == len(events) and same_info(im, it), (call, im, it)
        call += 1
        done += len(events)
        if done % 100 == 0:
            bind, slots = mixed.bindings()
            assert list(bind) == list(twin.bindings()[0])
            live = [i for i in range(slots) if (bind == i).any()]
            for cs in ([live[0]], live[1:4], live[::5]):
                S.check_whatif_derivation(mixed, None, cs)
            assert mixed.snapshot_fingerprint() == mixed.snapshot_fingerprint(cold=True) == twin.snapshot_fingerprint()
    assert done >= 1000 and call >= 40
    mixed.close(); twin.close()


# ---------------------------------------------------------------------------------------------------------------- 3. every field crosses
def every_field_node(name):
    """A state node that uses every field of the state_node record: labels, three taints, the three resource lists with quantities above 2^31 milli-units,
    two host ports, two volume limits, two volumes."""
    return StateNode(name=name,
                     labels={W.LABEL_PROVISIONER: "default", LABEL_HOSTNAME: name, LABEL_ZONE: W.ZONES[1], "team": "storage", "empty-value": ""},
                     taints=[Taint("dedicated", "storage", "NoSchedule"), Taint("maintenance", "", "NoExecute"), Taint("soft", "x", "PreferNoSchedule")],
                     available={"cpu": "63900m", "memory": "240Gi", "pods": "108", "ephemeral-storage": "3000Gi"},      # 240Gi = 2.6e14 milli-units
                     capacity={"cpu": "64", "memory": "256Gi", "pods": "110", "ephemeral-storage": "3500Gi"},
                     daemonset_requests={"cpu": "100m", "memory": "5Gi"},                                                 # 5Gi = 5.4e12 milli-units > 2^31
                     host_ports=[HostPort(9100, "TCP", "0.0.0.0"), HostPort(53, "UDP", "10.0.0.7")],
                     volume_limits={W.EBS_DRIVER: 3, W.EFS_DRIVER: 7},
                     volumes=[Volume(W.EBS_DRIVER, "default/node-listed-0"), Volume(W.EFS_DRIVER, "default/rwx-0000")])


def every_field_pod(uid):
    """A pod that uses every feature the pod record grammar carries."""
    sel = LabelSelector({"app": "db"}, [Expr("tier", "In", ["gold", "silver"]), Expr("canary", "DoesNotExist", [])])
    return Pod(uid=uid, namespace="prod", creation_ts=(1 << 33) + 12345, labels={"app": "db", "tier": "gold", "my-label": "a"},
               node_selector={"team": "storage"},
               required_affinity=[[Expr(LABEL_ZONE, "In", [W.ZONES[0], W.ZONES[1]]), Expr("team", "Exists", [])], [Expr(LABEL_ZONE, "NotIn", [W.ZONES[2]])]],
               preferred_affinity=[PreferredTerm(10, [Expr(LABEL_ZONE, "In", [W.ZONES[1]])]), PreferredTerm(-3, [Expr("team", "NotIn", ["web"])])],
               tolerations=[Toleration("dedicated", "Equal", "storage", "NoSchedule"), Toleration("maintenance", "Exists", "", "NoExecute"), Toleration("", "Exists", "", "")],
               containers=[Container(requests={"cpu": "1500m", "memory": "6Gi"}, limits={"cpu": "2", "memory": "8Gi", "ephemeral-storage": "10Gi"},
                                     ports=[HostPort(5432, "TCP", ""), HostPort(8125, "UDP", "10.0.0.7")]),
                           Container(requests={"cpu": "250m"}, limits={"memory": "3Gi"})],
               init_containers=[Container(requests={"cpu": "2", "memory": "1Gi"}, limits={"cpu": "3"})],
               spread=[TopologySpreadConstraint(2, LABEL_ZONE, DO_NOT_SCHEDULE, sel), TopologySpreadConstraint(1, LABEL_HOSTNAME, SCHEDULE_ANYWAY, None)],
               affinity_required=[PodAffinityTerm(LABEL_ZONE, LabelSelector({"app": "cache"}), ["prod", "shared"])],
               affinity_preferred=[WeightedPodAffinityTerm(7, PodAffinityTerm(LABEL_ZONE, LabelSelector({}, [Expr("app", "Exists", [])])))],
               anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"app": "db"}), ["prod"])],
               anti_preferred=[WeightedPodAffinityTerm(50, PodAffinityTerm(LABEL_ZONE, None, ["prod"]))],
               volumes=[Volume(W.EBS_DRIVER, "prod/data-db-0"), Volume(W.EFS_DRIVER, "default/rwx-0000")])


def rich_snapshot():
    """A volume snapshot whose provisioner has limits (a state node's capacity counts against them) and that runs a daemonset (a state node's daemonset requests
    are taken off what the daemonset would still ask for): with these every field of a state-node record reaches the flattening."""
    its, prov, nodes0, bound0 = W.volume_snapshot(12, 6, 31, unowned=False)
    prov = dataclasses.replace(prov, limits={"cpu": "5000", "memory": "20000Gi"})
    snap, pn = W.snapshot_problem(its, prov, nodes0, bound0, True)
    snap = dataclasses.replace(snap, daemonset_pods=[Pod(uid="ds-0", tolerations=[Toleration("", "Exists", "", "")], containers=[Container(requests={"cpu": "200m", "memory": "6Gi"})])])
    return snap, pn, nodes0, bound0


def test_every_field_crosses():
    """One handmade NODE+ and handmade BINDs through both doors: every flattening of the snapshot and every what-if flattened on the host -- the candidate set with
    the new node makes the rich pods the pending batch, so each of their fields reaches the flat problem -- come out equal, and equal to a snapshot ingested afresh
    with that node and those pods listed.  That the equality has teeth is checked too: emptying any one field of the node or of the pod moves a fingerprint.  Then
    the pod leaves and comes back under a negative timestamp, and a node leaves."""
    snap, pn, nodes0, bound0 = rich_snapshot()
    node, pod = every_field_node("rich-node"), every_field_pod("rich-pod")
    # (a twin of the pod on the same node, created earlier but with the later uid: the queue order of the two is decided by the creation timestamps' high words)
    adds = [("node+", node), ("bind", "rich-node", pod), ("bind", "rich-node", dataclasses.replace(every_field_pod("rich-pod-b"), creation_ts=12345, volumes=[])),
            ("bind", nodes0[2].name, dataclasses.replace(every_field_pod("rich-pod-2"), volumes=[]))]
    sets = [[len(nodes0)], [2], [0, 2, len(nodes0)], []]

    def through(door, events):
        p = S.ParsedProblem(snap)
        info = p.apply(events, pn) if door == "text" else p.apply_block(events, pn)
        return p, info, fingerprints(p, "volumes") + flat_hashes(p, None, sets)

    text, it, ht = through("text", adds)
    block, ib, hb = through("block", adds)
    assert ib["applied"] == 4 and same_info(it, ib)
    assert hb == ht
    for what, obj, at in (("node", node, 0), ("pod", pod, 1)):
        for f in dataclasses.fields(obj):
            if f.name in ("name", "uid", "in_state", "containers", "volume_error"):
                continue
            v = getattr(obj, f.name)
            other = {str: "other", int: 0}.get(type(v), type(v)())
            events = list(adds)
            events[at] = events[at][:-1] + (dataclasses.replace(obj, **{f.name: other}),)
            q, _, h = through("block", events)
            q.close()
            assert h != hb, f"{what}.{f.name} does not reach the flattening: the comparison above would not see it lost"
    # ... and the snapshot a caller would have listed: the node's usage follows its pods (state/node.go updateForPod), its available resources shrink by the pods' requests
    nodes_now, bound_now, _ = W.cluster_after(nodes0, bound0, adds)
    for n, b, n0 in ((nodes_now[-1], bound_now[-1], node), (nodes_now[2], bound_now[2][len(bound0[2]):], nodes0[2])):
        n.volumes = n0.volumes + [v for p in b for v in p.volumes]
        n.host_ports = n0.host_ports + [hp for p in b for c in p.containers for hp in c.ports]
    fresh, fresh_pn = fresh_in_library_order(snap, nodes0, bound0, nodes_now, adds, True)
    fp = S.ParsedProblem(fresh)
    assert list(block.bindings()[0]) == fresh_pn
    assert block.snapshot_fingerprint() == fp.snapshot_fingerprint(fresh_pn)
    assert block.snapshot_fingerprint(volumes=True) == fp.snapshot_fingerprint(fresh_pn, volumes=True)
    assert flat_hashes(block, None, sets) == flat_hashes(fp, fresh_pn, sets)
    fp.close()
    later = [("unbind", "rich-pod"), ("bind", "rich-node", dataclasses.replace(pod, creation_ts=-5)), ("node-", nodes0[2].name)]
    it, ib = text.apply(later), block.apply_block(later)
    assert ib["applied"] == 3 and same_info(it, ib)
    assert fingerprints(text, "volumes") == fingerprints(block, "volumes")
    assert list(text.bindings()[0]) == list(block.bindings()[0])
    assert flat_hashes(text, None, sets[:1]) == flat_hashes(block, None, sets[:1])
    text.close(); block.close()


# ---------------------------------------------------------------------------------------------------------------- 4. what the door refuses
def raw_apply_block(parsed, block, flags=0, pod_node=None):
    """The C entry point as it is (the flag word as given): (return code, ksh_last_error, info[0..3])."""
    kh = S.libs()[1]
    db = S._DeltaBlock(block["n_events"], block["n_strings"], block["n_words"], block["str_off"].ctypes.data, block["str_bytes"].ctypes.data, block["words"].ctypes.data,
                       int(block.get("str_bytes_len", block["str_bytes"].size)))
    pn = None if pod_node is None else np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32))
    info = (ctypes.c_uint32 * 4)()
    kh.ksh_env_apply_block.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    rc = kh.ksh_env_apply_block(parsed._p, None if pn is None else pn.ctypes.data, ctypes.byref(db), flags, info)
    return rc, kh.ksh_last_error().decode(), [int(x) for x in info]


def malformed_blocks(good):
    """(name, block, text the error must carry) for every way the issue lists in which a block can be malformed.  `good` holds: NODE- <name> | BIND ... | UNBIND <uid>."""
    def variant(**kw):
        b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        b.update(kw)
        return b
    words, so = good["words"], good["str_off"]
    out = []
    w = words.copy(); w[1] = good["n_strings"]
    out.append(("string id out of range", variant(words=w), "event 0: pod block: string id out of range"))
    w = words.copy(); w[-1] = good["n_strings"] + 5
    out.append(("string id out of range in the last event", variant(words=w), "event 2"))
    s = so.copy(); s[1], s[2] = so[2], so[1]
    out.append(("str_off not ascending", variant(str_off=s), "not ascending"))
    out.append(("str_off[n] beyond str_bytes_len", variant(str_bytes_len=int(so[-1]) - 1), "beyond str_bytes_len"))
    out.append(("truncated record", variant(n_words=good["n_words"] - 1), "event 2"))
    out.append(("truncated inside the pod", variant(n_words=good["n_words"] - 4), "event 1"))
    out.append(("trailing words", variant(words=np.concatenate([words[:good["n_words"]], np.asarray([M.EVENT_UNBIND], dtype=np.uint32)]), n_words=good["n_words"] + 1), "event 3: trailing words"))
    w = words.copy(); w[2] = 9
    out.append(("unknown kind", variant(words=w), "event 1: unknown event kind 9"))
    w = words.copy(); w[0] = 0
    out.append(("kind 0", variant(words=w), "event 0: unknown event kind 0"))
    out.append(("n_events larger than the stream", variant(n_events=4), "event 3"))
    out.append(("n_events far larger than the stream", variant(n_events=1 << 30), "n_events"))
    out.append(("n_events smaller than the stream", variant(n_events=2), "event 2: trailing words"))
    w = words.copy(); w[4] = good["n_words"]      # the BIND's spec word count
    out.append(("a pod record running past n_words", variant(words=w), "event 1"))
    return out


@pytest.mark.parametrize("first_call", [False, True])
def test_a_malformed_block_applies_nothing(first_call):
    """Each malformed block: KS_ERR_INVALID, the event's index in ksh_last_error(), info all zero, fingerprint and bindings as before -- also when the leading
    events of the block were fine, and also on a first call (the bindings are not taken over either)."""
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    rs = np.random.RandomState(0)
    if not first_call:
        assert parsed.apply_block([("bind", nodes[0].name, W.generic_pod(rs, "early"))], pn)["applied"] == 1
    fpn = pn if first_call else None      # (once events were applied the library holds the bindings)
    before = parsed.snapshot_fingerprint(fpn), parsed.snapshot_fingerprint(fpn, cold=True)
    bind_before = None if first_call else list(parsed.bindings()[0])
    good = M.delta_to_block([("node-", nodes[3].name), ("bind", nodes[1].name, W.generic_pod(rs, "late")), ("unbind", bound[2][0].uid)])
    assert int(good["words"][0]) == M.EVENT_NODE_REMOVE and int(good["words"][2]) == M.EVENT_BIND and int(good["words"][-2]) == M.EVENT_UNBIND
    for name, blk, needle in malformed_blocks(good):
        rc, msg, info = raw_apply_block(parsed, blk, pod_node=fpn)
        assert rc == S.KS_ERR_INVALID and needle in msg and "delta block" in msg, (name, rc, msg)
        assert info == [0, 0, 0, 0], (name, info)
        assert (parsed.snapshot_fingerprint(fpn), parsed.snapshot_fingerprint(fpn, cold=True)) == before, name
        if first_call:
            with pytest.raises(S.KSolveError, match="no ksh_env_apply yet"):
                parsed.bindings()
        else:
            assert list(parsed.bindings()[0]) == bind_before, name
    for flags in (2, 1 << 16, 0x80000000, 3):      # any bit but KSH_APPLY_TRACK_CLUSTER_PODS
        rc, msg, info = raw_apply_block(parsed, good, flags=flags, pod_node=fpn)
        assert rc == S.KS_ERR_INVALID and "flag" in msg and info == [0, 0, 0, 0], (flags, msg)
        assert (parsed.snapshot_fingerprint(fpn), parsed.snapshot_fingerprint(fpn, cold=True)) == before
    with pytest.raises(S.KSolveError) as ei:      # (the Python mirror raises the same refusal)
        parsed.apply_block(malformed_blocks(good)[0][1], fpn)
    assert ei.value.code == S.KS_ERR_INVALID and ei.value.info["applied"] == 0
    # ... and the block as it was is taken
    rc, msg, info = raw_apply_block(parsed, good, pod_node=fpn)
    assert rc == S.KS_OK and info[0] == 3, msg
    assert parsed.snapshot_fingerprint() != before[0]
    parsed.close()


@pytest.mark.parametrize("bad,needle", [(("node-", "nobody"), "event 2: NODE-: no state node named nobody"), (("unbind", "nobody"), "event 2: UNBIND: no bound pod with uid nobody")])
def test_an_event_that_cannot_be_applied_keeps_the_ones_before(bad, needle):
    """A block that decodes but whose third event names nothing the snapshot has: as in `ksh_env_apply`, KS_ERR_INVALID with the text door's words, info[0] == 2,
    and the two good events stay -- the snapshot equals one that heard only those two."""
    its, prov, nodes, bound = W.cluster_snapshot(8, 6, 5)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed, two, text = S.ParsedProblem(snap), S.ParsedProblem(snap), S.ParsedProblem(snap)
    for p in (parsed, two, text):
        p.snapshot_fingerprint(pn)
    rs = np.random.RandomState(1)
    good = [("node+", W.fresh_node(its, "joined", rs)), ("bind", "joined", W.generic_pod(rs, "on-joined"))]
    with pytest.raises(S.KSolveError) as ei:
        parsed.apply_block(good + [bad, ("unbind", bound[0][0].uid)], pn)
    assert ei.value.code == S.KS_ERR_INVALID and needle in str(ei.value) and "the events before it were applied" in str(ei.value)
    assert ei.value.info["applied"] == 2 and ei.value.info["nodes"] == 9 and ei.value.info["pods"] == len(pn) + 1
    with pytest.raises(S.KSolveError) as et:      # the text door: the same words
        text.apply(good + [bad, ("unbind", bound[0][0].uid)], pn)
    assert str(et.value) == str(ei.value)
    assert two.apply_block(good, pn)["applied"] == 2
    assert parsed.snapshot_fingerprint() == two.snapshot_fingerprint() == text.snapshot_fingerprint() == parsed.snapshot_fingerprint(cold=True)
    assert list(parsed.bindings()[0]) == list(two.bindings()[0]) == list(text.bindings()[0])
    assert parsed.bindings()[0][-1] == 8
    for p in (parsed, two, text):
        p.close()


def test_spare_room_used_up_is_the_text_doors_refusal():
    """The snapshot was ingested with room for 256 more nodes: the 257th NODE+ of one block is refused as in `ksh_env_apply`, the 256 before it stay."""
    its, prov, nodes, bound = W.cluster_snapshot(4, 4, 2)
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    rs = np.random.RandomState(2)
    with pytest.raises(S.KSolveError, match="event 256: NODE\\+: the snapshot's spare room for nodes is used up") as ei:
        parsed.apply_block([("node+", W.fresh_node(its, f"more-{k}", rs)) for k in range(300)], pn)
    assert ei.value.info["applied"] == 256 and ei.value.info["nodes"] == 260
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- 5. KSH_APPLY_TRACK_CLUSTER_PODS
def test_track_cluster_pods_flag():
    """A topology-tracking snapshot that starts with NO bound pods, then 30 BINDs of spread pods.  Whether `ksh_env_apply` mirrors bound pods into the cluster pods
    (what countDomains counts, topology.go:231-276) is inferred from "the snapshot had some at the first call"; the new door lets the caller say it.  With the flag
    the host-flattened what-ifs equal those over a snapshot ingested afresh with the pods and cluster pods listed; without it the door does what the text door does."""
    its, prov, nodes, _ = W.cluster_snapshot(12, 6, 91)
    empty = [[] for _ in nodes]
    snap, pn = W.snapshot_problem(its, prov, nodes, empty, True)
    assert not snap.pods and not snap.cluster_pods
    rs = np.random.RandomState(4)
    binds = [("bind", nodes[int(rs.randint(len(nodes)))].name, spread_pod(rs, f"spread-{k}")) for k in range(30)]
    flagged, plain, text = S.ParsedProblem(snap), S.ParsedProblem(snap), S.ParsedProblem(snap)
    for lo in range(0, 30, 10):      # (three calls: the flag is the caller's word on every call)
        assert flagged.apply_block(binds[lo:lo + 10], track_cluster_pods=True)["applied"] == 10
        assert plain.apply_block(binds[lo:lo + 10])["applied"] == 10
        assert text.apply(binds[lo:lo + 10])["applied"] == 10
    nodes_now, bound_now, _ = W.cluster_after(nodes, empty, binds)
    fresh, fresh_pn = fresh_in_library_order(snap, nodes, empty, nodes_now, binds, True)
    assert len(fresh.cluster_pods) == 30
    fp = S.ParsedProblem(fresh)
    sets = [[i] for i in range(len(nodes))] + [[0, 1, 2, 3], list(range(0, len(nodes), 2))]
    want = flat_hashes(fp, fresh_pn, sets)
    assert list(flagged.bindings()[0]) == fresh_pn
    assert flat_hashes(flagged, None, sets) == want
    assert flagged.snapshot_fingerprint() == fp.snapshot_fingerprint(fresh_pn)
    assert flat_hashes(plain, None, sets) == flat_hashes(text, None, sets)
    assert plain.snapshot_fingerprint() == text.snapshot_fingerprint()
    # UNBIND / NODE- take the mirrored pods out again under the flag
    leave = [("unbind", "spread-3"), ("unbind", "spread-17"), ("node-", nodes[5].name)]
    assert flagged.apply_block(leave, track_cluster_pods=True)["applied"] == 3
    nodes2, bound2, slot = W.cluster_after(nodes, empty, binds + leave)
    fresh2, fresh2_pn = W.snapshot_problem(its, prov, nodes2, bound2, True)
    fp2 = S.ParsedProblem(fresh2)
    for cs in ([0], [1, 2, 3], list(range(0, len(nodes2), 2))):
        S.check_whatif_derivation(flagged, None, [slot[i] for i in cs])
        S.check_whatif_derivation(fp2, fresh2_pn, cs)
    for p in (flagged, plain, text, fp, fp2):
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the door from plain C
def test_delta_block_from_plain_c(tmp_path):
    """tests/cabi_usage_delta.c -- a two-event block built by hand, applied, compared with the text door; a block whose n_events does not match refused -- compiled as
    C99 with -Wall -Werror -pedantic against include/kshost.h, linked against both libraries and run (no GPU needed)."""
    import __graft_entry__ as ge
    ge.build()
    pkg = os.path.join(ROOT, "karpenter_core_amd")
    exe = str(tmp_path / "cabi_usage_delta")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_delta.c"),
                           "-o", exe, "-L", pkg, "-lkshost", "-lksolve", "-Wl,-rpath," + pkg])
    env_file = tmp_path / "env.ksp"
    env_file.write_text(dataclasses.replace(W.config1(pods=1, types=5), pods=[]).to_ksp())
    out = subprocess.run([exe, str(env_file)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "refused: delta block: event 2" in out.stdout
    assert "applied 2 events: 1 nodes 1 pods" in out.stdout
    assert "binary and text door: the same flattening" in out.stdout
    syms = subprocess.run(["nm", "-D", os.path.join(pkg, "libkshost.so")], capture_output=True, text=True).stdout
    assert " T ksh_env_apply_block" in syms and " T ksh_env_apply\n" in syms


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("seed,kind", [(21, "plain"), (22, "plain"), (23, "topology"), (24, "topology"), (25, "volumes"), (26, "volumes")])
def test_whatifs_over_the_block_patched_snapshot_solve_like_a_fresh_one(seed, kind):
    """`test_env_apply.test_whatifs_over_the_patched_snapshot_solve_like_a_fresh_one` for the new door: the snapshot is flattened and resident, 30 events arrive
    through `apply_block` (continuing that flattening) and through `apply` into a twin; the what-ifs DERIVED on the device over the two, and over a snapshot built
    fresh from the cluster as it is now, solve to the same results, reasons included -- and to the oracle's on a sample."""
    from oracle import oracle_py as O
    volumes = kind == "volumes"
    its, prov, nodes0, bound0, cps, make = make_cluster(kind, 64, 10, 300 + seed, spare_pod_slots=(6 if seed % 2 else -1))
    snap, pn = W.snapshot_problem(its, prov, nodes0, bound0, cps)
    parsed, twin = S.ParsedProblem(snap), S.ParsedProblem(snap)
    rs = np.random.RandomState(seed)
    for p in (parsed, twin):
        for f in S.open_whatifs(p, pn, [[0], [1, 2], [5]], derive=True, volumes=volumes):      # (flattened and resident BEFORE the events: they continue that flattening)
            f.close()
    all_events, nodes, bound = [], nodes0, bound0
    for batch in range(3):
        events, nodes, bound = events_for(kind, rs, its, nodes, bound, 10, f"g{seed}b{batch}", make)
        ib = parsed.apply_block(events, pn if batch == 0 else None)
        it = twin.apply(events, pn if batch == 0 else None)
        assert ib["continued"] and same_info(ib, it)
        all_events += events
    assert parsed.snapshot_fingerprint(volumes=volumes) == twin.snapshot_fingerprint(volumes=volumes)
    # the cluster as it is now, the way a caller would list it; its node j sits in the library's slot slot_of[j]
    nodes, bound, slot_of = after(kind, nodes0, bound0, all_events)
    fresh_snap, fresh_pn = W.snapshot_problem(its, prov, nodes, bound, cps)
    fresh = S.ParsedProblem(fresh_snap)
    sets = [[int(x) for x in rs.choice(len(nodes), size=int(rs.choice([1, 1, 2, 4, 8])), replace=False)] for _ in range(24)]
    slots = [[slot_of[j] for j in cs] for cs in sets]
    got_f = S.open_whatifs(parsed, None, slots, derive=True, volumes=volumes)
    twin_f = S.open_whatifs(twin, None, slots, derive=True, volumes=volumes)
    want_f = S.open_whatifs(fresh, fresh_pn, sets, derive=True, volumes=volumes)
    try:
        got, _, _ = S.solve_batch(got_f)
        via_text, _, _ = S.solve_batch(twin_f)
        want, _, _ = S.solve_batch(want_f)
        for i, (g, t, w) in enumerate(zip(got, via_text, want)):
            assert g.canonical() == t.canonical() and g.reasons == t.reasons, (seed, i, sets[i])
            assert g.canonical() == w.canonical() and g.reasons == w.reasons, (seed, i, sets[i])
        for i in range(0, len(sets), 6):
            ref = O.solve(W.whatif(its, prov, nodes, bound, sets[i], cps))
            assert got[i].canonical() == ref.canonical(), (seed, i, sets[i])
    finally:
        for f in got_f + twin_f + want_f:
            f.close()
        parsed.close(); twin.close(); fresh.close()
