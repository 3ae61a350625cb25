"""Consolidation commands decided on the device (include/kshost.h ksh_consolidation_commands / ksh_first_n_node_option / ksh_single_node_option; kernel
ks_consolidation_commands in csrc/ksolve.hip) against the literal restatement in oracle/consolidation_ref.py, one oracle Solve per probe.

The snapshots are the ones tests/test_consolidation.py builds (imported, not copied), price catalogues of tests/test_price_stage.py turned into snapshots whose
candidates cost exactly a worst launch price and one ulp more, and handmade ones for the branches nothing else reaches.  Every case runs twice, as in
tests/test_price_stage.py: unmarked on the emulator build of the kernels (tests/sim) in a child process, and marked `gpu` on the device.  `device_run` is the part
that needs the kernels; every comparison happens here, against the oracle.  `consolidation.py`'s own route is compared too on the device leg, as a second opinion."""
import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import consolidation as C, fake
from karpenter_core_amd.model import (LABEL_CAPACITY_TYPE as CT, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_PROVISIONER, LABEL_ZONE as ZONE, Container, Offering, Pod, Problem,
                                      StateNode)
from oracle import consolidation_ref as CR
from oracle import oracle_py as O

import test_consolidation as TC
import test_price_stage as TP

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DO_NOTHING, DELETE, REPLACE, ERROR = 0, 1, 2, 3
WHY_NOT_ALL_SCHEDULED, WHY_MANY_NODES, WHY_PRICE_ERROR, WHY_NOT_CHEAPER, WHY_SPOT_TO_SPOT, WHY_SAME_TYPE, WHY_DELETING = 1, 3, 4, 6, 7, 9, 10
ACTIONS = {"do-nothing": DO_NOTHING, "delete": DELETE, "replace": REPLACE}
F_BLOCKED, F_ALL_SPOT, F_PRICE_ERROR, F_SAME_TYPE = 1, 2, 4, 8
POISON = 0xA5A5A5A5DEADBEEF


# ---------------------------------------------------------------------------------------------------------------- the cases
def _zonal_spread():
    from karpenter_core_amd.model import DO_NOT_SCHEDULE, LabelSelector, TopologySpreadConstraint
    its = fake.instance_types_assorted()
    nodes = TC._zonal_nodes(its, most_expensive_zone="test-zone-2")
    labels = {"app": "test-zonal-spread"}
    bound = [[Pod(uid=f"p{i}", labels=dict(labels), containers=[Container(requests={"cpu": "1"})],
                  spread=[TopologySpreadConstraint(1, ZONE, DO_NOT_SCHEDULE, LabelSelector(dict(labels)))])] for i in range(3)]
    return TC.snapshot(its, nodes, bound)


def _anti_affinity():
    from karpenter_core_amd.model import LabelSelector, PodAffinityTerm
    its = fake.instance_types_assorted()
    nodes = TC._zonal_nodes(its)
    labels = {"app": "test"}
    bound = [[Pod(uid=f"p{i}", labels=dict(labels), containers=[Container(requests={"cpu": "1"})],
                  anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector(dict(labels)))])] for i in range(3)]
    return TC.snapshot(its, nodes, bound)


def _pending_and_deleting(deleting, pending):
    snap = TC._pending_and_deleting()
    snap.deleting, snap.pending = tuple(deleting), [TC.pod(u, c) for u, c in pending]
    return snap


def _busy(existing, seed, util, deleting=(), pending=0):
    snap = TC.busy_cluster(existing, seed, util=tuple(util))
    snap.deleting, snap.pending = tuple(deleting), [TC.pod(f"pend-{i}", "1") for i in range(pending)]
    return snap


def _handmade():
    """The branches no restated scenario reaches.  Four types: `spot-cheap` (spot only), `od-cheap` (on-demand only), `both` (spot and on-demand), `big` (what the
    candidates run on).  n-spot is a spot node whose pod takes any capacity type: the replacement Has(spot) -> "can't replace a spot node with a spot node".  n-od's pod
    takes any capacity type too: the replacement Has(spot) and Has(on-demand) -> narrowed to spot.  n-od-pin's pod insists on on-demand: no narrowing.  n-two carries two
    pods that exclude each other's zones: two new nodes.  n-huge's pod fits nothing: unscheduled."""
    its = [fake.new_instance_type("spot-cheap", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("spot", "z-a", 0.1, True), Offering("spot", "z-b", 0.15, True)]),
           fake.new_instance_type("od-cheap", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("on-demand", "z-a", 0.3, True), Offering("on-demand", "z-b", 0.35, True)]),
           fake.new_instance_type("both", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("spot", "z-a", 0.2, True), Offering("on-demand", "z-a", 0.5, True)]),
           fake.new_instance_type("big", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("spot", "z-a", 0.9, True), Offering("on-demand", "z-a", 2.0, True), Offering("on-demand", "z-b", 2.0, True)])]
    big = its[3]

    def full(name, ct, zone):        # a node with no room left: whatever leaves it needs a new node
        n = TC.node(name, big, ct, zone, cpu="4")
        n.available = {"cpu": "0", "pods": "10"}
        return n
    from karpenter_core_amd.model import Expr
    pin = TC.pod("p-od-pin")
    pin.node_selector = {CT: "on-demand"}
    pa, pb = TC.pod("p-two-a"), TC.pod("p-two-b")
    pa.required_affinity, pb.required_affinity = [[Expr(ZONE, "In", ["z-a"])]], [[Expr(ZONE, "In", ["z-b"])]]
    nodes = [full("n-spot", "spot", "z-a"), full("n-od", "on-demand", "z-a"), full("n-od-pin", "on-demand", "z-a"), full("n-two", "on-demand", "z-b"), full("n-huge", "on-demand", "z-a")]
    bound = [[TC.pod("p-spot")], [TC.pod("p-od")], [pin], [pa, pb], [TC.pod("p-huge", "64")]]
    return TC.snapshot(its, nodes, bound)


def _same_type_kept_and_emptied():
    """filterOutSameType both ways.  Candidates on `mid` (1.0) and `top` (3.0), one pod each, together they fit `mid` or `low`: the replacement options are {low, mid}
    (both cheaper than 4.0), `mid` is a candidate's own type at 1.0 -> the second stage keeps only what is cheaper than 1.0: {low}.  With `low` absent from the
    catalogue the second stage empties."""
    def cat(with_low):
        its = [fake.new_instance_type("mid", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("on-demand", "z-a", 1.0, True)]),
               fake.new_instance_type("top", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("on-demand", "z-a", 3.0, True)])]
        if with_low:
            its.insert(0, fake.new_instance_type("low", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("on-demand", "z-a", 0.5, True)]))
        return its
    out = {}
    for tag, with_low in (("kept", True), ("emptied", False)):
        its = cat(with_low)
        by = {it.name: it for it in its}
        nodes = [TC.node("n-mid", by["mid"], "on-demand", "z-a", cpu="4"), TC.node("n-top", by["top"], "on-demand", "z-a", cpu="4")]
        for n in nodes:
            n.available = {"cpu": "0", "pods": "10"}
        pods = [TC.pod("p-mid"), TC.pod("p-top")]
        for p in pods:
            p.node_selector = {CT: "on-demand"}          # (no narrowing to spot: the second stage prices on-demand)
        out[tag] = TC.snapshot(its, nodes, [[pods[0]], [pods[1]]])
    return out


NC = 8       # candidate price types a price snapshot adds to its catalogue


def price_snapshot(spec, pods=5):
    """A price catalogue of tests/test_price_stage.py as a snapshot: `pods` of its pods, each alone on full nodes -- one node per candidate price --, so that every
    singleton what-if opens exactly one new node with that pod's zone / capacity-type requirements.  The candidate prices are worst launch prices of that node's
    options and the next double above each (filterByPrice compares with a strict <): node n-<pod>-<k> runs on the instance type cand-<k>, whose only offering is
    UNAVAILABLE (never a replacement option; Offerings.Get does not consult availability) at exactly that price.  T = the catalogue's types + NC."""
    pr = TP.build_problem(spec)
    zs = sorted({o.zone for it in pr.instance_types for o in it.offerings})
    prices, per_pod = [], []
    for p in pr.pods[:pods]:
        ref = O.solve(Problem(instance_types=pr.instance_types, provisioners=pr.provisioners, pods=[p], extra_well_known=pr.extra_well_known))
        worst = sorted(set(TP.worst_prices(pr, ref.new_nodes[0], False).values())) if ref.new_nodes else []
        mine = []
        for w in worst:
            for c in (w, math.nextafter(w, math.inf)):
                if c not in prices and len(prices) < NC and c < CR.MAX_FLOAT64:
                    prices.append(c)
                if c in prices and prices.index(c) not in mine:
                    mine.append(prices.index(c))
        per_pod.append(mine[:4] or [0])
    while len(prices) < NC:
        prices.append(7.0 + len(prices))
    cand_types = [fake.new_instance_type(f"cand-{k}", {"cpu": "1", "memory": "1Gi", "pods": "4"}, [Offering("on-demand", zs[0], c, False)]) for k, c in enumerate(prices)]
    its = list(pr.instance_types) + cand_types
    nodes, bound = [], []
    for i, (p, ks) in enumerate(zip(pr.pods[:pods], per_pod)):
        for k in ks:
            name = f"n-{i}-{k}"
            labels = {LABEL_PROVISIONER: "default", LABEL_INSTANCE_TYPE: f"cand-{k}", CT: "on-demand", ZONE: zs[0], LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
            nodes.append(StateNode(name=name, labels=labels, available={"cpu": "0", "memory": "0", "pods": "4"}, capacity={"cpu": "1", "memory": "1Gi", "pods": "4"}))
            q = copy.deepcopy(p)
            q.uid = f"{p.uid}-{k}"
            bound.append([q])
    return C.Snapshot(its, fake.provisioner("default", len(its)), nodes, bound)


PRICE = {
    "price-spot_on_demand-1": ("catalogue", {"seed": 1}),
    "price-third_capacity_type-11": ("catalogue", {"seed": 11, "cts": ("spot", "on-demand", "reserved")}),
    "price-no_spot-21": ("catalogue", {"seed": 21, "cts": ("on-demand",)}),
    "price-pairs_64-37": ("catalogue", {"seed": 37, "zones": 32, "types": 48, "pods": 60}),
    "price-types_65-41": ("catalogue", {"seed": 41, "types": 65 - NC}),
    "price-tw_over_64-51": ("catalogue", {"seed": 51, "types": 4160, "pods": 24}),
    "price-duplicate_pairs": ("duplicate_pairs", {}),
    "price-unavailable_offerings": ("unavailable_offerings", {}),
    "price-ties": ("ties", {}),
}

_BUILT = {}


def case(name):
    """-> (snapshot, candidate sets for computeConsolidation, candidate list for the two searches or None); built once per process"""
    if name in _BUILT:
        return _BUILT[name]
    if name.startswith("price-"):
        snap = price_snapshot(PRICE[name], pods=3 if "tw_over" in name else 5)
        out = (snap, [[i] for i in range(len(snap.nodes))], None)
    elif name.startswith("scenario-"):
        snap, cands, _ = TC.scenarios()[name[9:]]
        out = (snap, [cands] + [[c] for c in range(len(snap.nodes)) if [c] != cands], list(range(len(snap.nodes))))
    elif name.startswith("multi-"):
        snap, cands, _, _ = TC.multi_scenarios()[name[6:]]
        out = (snap, [cands[:k] for k in range(1, len(cands) + 1)], cands)
    elif name == "uninitialized_neighbour":
        snap, cands = TC._uninitialized_neighbour()
        out = (snap, [cands, [1], [0, 1]], [0, 1])
    elif name == "missing_offering":
        snap, cands = TC._missing_offering()
        out = (snap, [[0], [1], [0, 1]], cands)
    elif name.startswith("pending_deleting-"):
        deleting, pending = {"a": ((), []), "b": ((2,), []), "c": ((), [("q0", "2"), ("q1", "2")]), "d": ((1,), [("q0", "1")])}[name[-1]]
        out = (_pending_and_deleting(deleting, pending), [[0], [1], [2], [0, 1]], [0, 1, 2])
    elif name == "zonal_spread":
        out = (_zonal_spread(), [[0], [1], [2], [0, 1]], [0, 1, 2])
    elif name == "anti_affinity":
        out = (_anti_affinity(), [[0], [1], [2], [0, 1, 2]], [0, 1, 2])
    elif name.startswith("busy-"):
        seed = int(name[5:])
        if seed == 5:        # tests/test_consolidation.py: pending pods and two deleting nodes
            snap = _busy(24, 5, (0.9, 0.99), deleting=(3, 17), pending=6)
            cands = [i for i in range(12) if i not in snap.deleting]
        elif seed == 60:     # the roomy cluster: the binary search finds a multi-node replace
            snap = _busy(60, 11, (0.75, 0.98))
            cands = [int(x) for x in np.random.RandomState(11).choice(len(snap.nodes), size=16, replace=False)]
        else:
            snap = _busy(24, seed, (0.93, 0.999))
            cands = [int(x) for x in np.random.RandomState(seed).choice(len(snap.nodes), size=12, replace=False)]
        out = (snap, [[c] for c in cands] + [cands[:k] for k in range(2, len(cands) + 1)], cands)
    elif name == "volumes":
        # CSI volume limits and claims: without KSH_DERIVE_VOLUMES the derivation is refused and the call flattens the what-ifs one by one, with it they are derived
        from karpenter_core_amd import workloads as W
        its, prov, nodes, bound = W.volume_snapshot(24, 6, 45, unowned=False)
        for i, n in enumerate(nodes):       # a tight cluster: only one node in eight has cpu left, so that most of what leaves a node needs a new one
            if i % 8:
                n.available = dict(n.available, cpu="0")
        snap = C.Snapshot(its, prov, nodes, bound)
        cands = [int(x) for x in np.random.RandomState(45).choice(len(nodes), size=8, replace=False)]
        out = (snap, [[c] for c in cands] + [cands[:3]], cands)
    elif name == "handmade":
        snap = _handmade()
        out = (snap, [[0], [1], [2], [3], [4], [0, 1]], [0, 1, 2])
    elif name.startswith("same_type-"):
        snap = _same_type_kept_and_emptied()[name[10:]]
        out = (snap, [[0], [1], [0, 1]], [0, 1])
    else:
        raise KeyError(name)
    _BUILT[name] = out
    return out


CASES = ([f"scenario-{n}" for n in sorted(TC.scenarios())] + [f"multi-{n}" for n in sorted(TC.multi_scenarios())] +
         ["uninitialized_neighbour", "missing_offering", "pending_deleting-a", "pending_deleting-b", "pending_deleting-c", "pending_deleting-d", "zonal_spread", "anti_affinity",
          "busy-3", "busy-11", "busy-5", "busy-60", "volumes", "handmade", "same_type-kept", "same_type-emptied"] + list(PRICE))


# ---------------------------------------------------------------------------------------------------------------- the device side
def host_inputs(snap, cs, same_type):
    """What the library builds from the parsed nodes' labels, restated: (KS_CMD_F_* flags, getNodePrices, [(type index, lowest candidate price or 0.0)])."""
    tindex = {it.name: i for i, it in enumerate(snap.instance_types)}
    types = {it.name: it for it in snap.instance_types}
    flags, price, lows = (F_SAME_TYPE if same_type else 0), 0.0, {}
    cands = [CR.Cand(snap, i) for i in cs]
    for c in cands:
        o = CR.offering_get(types[c.instance_type], c.capacity_type, c.zone)
        lows.setdefault(c.instance_type, None)
        if o is None:
            flags |= F_PRICE_ERROR
            continue
        price += o.price
        lows[c.instance_type] = o.price if lows[c.instance_type] is None else min(lows[c.instance_type], o.price)
    if all(c.capacity_type == "spot" for c in cands):
        flags |= F_ALL_SPOT
    gone = set(cs) | set(snap.deleting)
    if any(n.in_state and n.owned and n.labels.get("karpenter.sh/initialized") != "true" for j, n in enumerate(snap.nodes) if j not in gone):
        flags |= F_BLOCKED
    return flags, price, [(tindex[n], 0.0 if p is None else p) for n, p in lows.items()]


def _jsonable(d):
    d = dict(d)
    d["requirements"] = {k: [v[0], list(v[1]), v[2], v[3]] for k, v in d["requirements"].items()}
    return d


def device_run(S, name):
    """One case on one backend.  Plain data out: the decoded rows of ksh_consolidation_commands (plain and with filterOutSameType), the two searches, and the row
    hygiene of the handle route (poisoned buffer, words > TW, shuffled ids, twice)."""
    snap, sets, multi = case(name)
    words = (len(snap.instance_types) + 63) // 64
    parsed, pod_node, leaving = C._command_snapshot(snap)
    out = {}
    try:
        for tag, same in (("plain", False), ("same_type", True)):
            rows, _ = S.consolidation_commands(parsed, pod_node, sets, words, deleting=leaving, same_type=same)
            out[tag] = [_jsonable(S.decode_command_row(parsed, rows[i], words)) for i in range(len(sets))]
            out[tag + "_cmd"] = [list(C._command_of_row(snap, parsed, rows[i], words, cs).canonical()) if (int(rows[i][1]) & 0xFF) != ERROR else "error" for i, cs in enumerate(sets)]
            out[tag + "_hex"] = [rows[i].tobytes().hex() for i in range(len(sets))]
        if name == "volumes":       # the routes the flags choose: derived with the volumes, and over the active resource names; all must give the plain call's rows
            for tag, kw in (("derive_volumes", {"volumes": True}), ("active_resources", {"active_resources": True}), ("both_flags", {"volumes": True, "active_resources": True})):
                rows, _ = S.consolidation_commands(parsed, pod_node, sets, words, deleting=leaving, same_type=True, **kw)
                out[tag + "_hex"] = [rows[i].tobytes().hex() for i in range(len(sets))]
            try:
                S.open_whatifs(parsed, pod_node, sets, derive=True)
                out["derivation_refused_without_flag"] = False
            except S.KSolveError as e:
                out["derivation_refused_without_flag"] = e.code == S.KS_ERR_UNSUPPORTED
            fl = S.open_whatifs(parsed, pod_node, sets, derive=True, volumes=True)
            out["derived_with_flag"] = len(fl) == len(sets)
            for f in fl:
                f.close()
        if multi is not None:
            try:
                out["first_n"] = list(C.first_n_node_consolidation_option_dev(snap, multi).canonical())
            except ValueError:
                out["first_n"] = "error"
            out["single"] = list(C.single_node_consolidation_option_dev(snap, multi).canonical())
            if getattr(S, "_SIM_ACTIVE", False) is False:        # the device leg: consolidation.py's own route, as a second opinion
                try:
                    out["py_first_n"] = list(C.first_n_node_consolidation_option(snap, multi).canonical())
                except ValueError:
                    out["py_first_n"] = "error"
                out["py_single"] = list(C.single_node_consolidation_option(snap, multi).canonical())
        # the handle route over the live what-ifs: the same rows, whatever the buffer held before and however wide the rows are
        live = [i for i, cs in enumerate(sets) if not (set(cs) & set(snap.deleting))]
        pend = [j for j in leaving if j >= len(snap.nodes)]
        flats = S.open_whatifs(parsed, pod_node, [pend + list(sets[i]) + [int(j) for j in snap.deleting] for i in live])
        try:
            S.solve_batch_resident(flats)
            order = [int(x) for x in np.random.RandomState(len(live)).permutation(len(live))]
            wide = words + 3
            calls = []
            for _ in range(2):
                buf = np.full((max(1, len(live)), S.command_row_words(wide)), POISON, dtype=np.uint64)
                ins = [host_inputs(snap, sets[live[k]], True) for k in order]
                rows = S.command_rows([flats[k] for k in order], [live[k] for k in order], [x[0] for x in ins], [x[1] for x in ins], [x[2] for x in ins], wide, out=buf)
                calls.append(rows)
            out["hygiene"] = {"same_bytes": calls[0].tobytes() == calls[1].tobytes(), "poison_left": int((calls[0] == np.uint64(POISON)).sum()), "ids": [int(r[0]) for r in calls[0]],
                              "want_ids": [live[k] for k in order],
                              "tails_zero": bool((calls[0][:, 72 + words:72 + wide] == 0).all() and (calls[0][:, 72 + wide + words:] == 0).all()),
                              "narrow": [calls[0][i, :72].tobytes().hex() + calls[0][i, 72:72 + words].tobytes().hex() + calls[0][i, 72 + wide:72 + wide + words].tobytes().hex() for i in range(len(live))],
                              "live_in_order": [live[k] for k in order]}
        finally:
            for f in flats:
                f.close()
    finally:
        parsed.close()
    return out


def map_miss_run(S):
    """The Go map miss of multinodeconsolidation.go:150-158 at the kernel: a listed type priced 0.0 (no candidate of it had an offering) that stage 1 kept makes the
    second ceiling 0.0.  computeConsolidation never lets such a set through (getNodePrices fails first), so the inputs are given by hand over the handle route."""
    snap, _ = TC._missing_offering()
    words = (len(snap.instance_types) + 63) // 64
    parsed, pod_node, _ = C._command_snapshot(snap)
    flats = S.open_whatifs(parsed, pod_node, [[0]])
    try:
        S.solve_batch_resident(flats)
        _, _, lst = host_inputs(snap, [0], True)
        rows = S.command_rows(flats, [0], [F_SAME_TYPE], [CR.MAX_FLOAT64], [lst], words)
        free = S.command_rows(flats, [0], [F_SAME_TYPE], [CR.MAX_FLOAT64], [[]], words)
        return {"listed": lst, "row": _jsonable(S.decode_command_row(parsed, rows[0], words)), "unlisted": _jsonable(S.decode_command_row(parsed, free[0], words))}
    finally:
        for f in flats:
            f.close()
        parsed.close()


MIXED = ["price-spot_on_demand-1", "price-types_65-41", "price-ties"]


def mixed_t_run(S):
    """One command call over what-ifs of snapshots with different T (the handle route: the rows are as wide as the widest)."""
    opened, flats, ins, ids, per = [], [], [], [], []
    try:
        for k, name in enumerate(MIXED):
            snap, sets, _ = case(name)
            parsed, pod_node, _ = C._command_snapshot(snap)
            opened.append(parsed)
            fl = S.open_whatifs(parsed, pod_node, sets)
            S.solve_batch_resident(fl)
            flats += fl
            ins += [host_inputs(snap, cs, False) for cs in sets]
            ids += [k * 1000 + i for i in range(len(sets))]
            per.append((len(snap.instance_types) + 63) // 64)
        wide = max(per)
        rows = S.command_rows(flats, ids, [x[0] for x in ins], [x[1] for x in ins], [x[2] for x in ins], wide)
        out, at = [], 0
        for k, name in enumerate(MIXED):
            n = len(case(name)[1])
            out.append([_jsonable(S.decode_command_row(opened[k], rows[at + i], wide)) for i in range(n)])
            at += n
        return {"rows": out, "words": per}
    finally:
        for f in flats:
            f.close()
        for p in opened:
            p.close()


def refusals_run(S):
    """Every refusal's return code and message; then the same handles still answer."""
    snap, sets, _ = case("scenario-can_replace_node")
    words = (len(snap.instance_types) + 63) // 64
    T = len(snap.instance_types)
    parsed, pod_node, _ = C._command_snapshot(snap)
    flats = S.open_whatifs(parsed, pod_node, [[0], [0]])
    out = {}

    def refused(tag, fn):
        try:
            fn()
            out[tag] = [0, ""]
        except S.KSolveError as e:
            out[tag] = [e.code, str(e)]
    try:
        S.solve_batch_resident(flats)
        good = lambda **kw: S.command_rows(flats, [0, 1], kw.get("flags", [0, 0]), [1.0, 1.0], kw.get("lists", [[(0, 1.0)], [(1, 1.0)]]), kw.get("words", words), type_off=kw.get("off"))
        before = good().tobytes()
        refused("words_short", lambda: good(words=words - 1))
        refused("type_index", lambda: good(lists=[[(0, 1.0)], [(T, 1.0)]]))
        refused("offsets", lambda: good(off=[0, 2, 1]))
        refused("flag_bit", lambda: good(flags=[0, 16]))
        refused("library_flag_bit", lambda: S.consolidation_commands(parsed, pod_node, [[0]], words, flags=1 << 20))
        refused("library_words_short", lambda: S.consolidation_commands(parsed, pod_node, [[0]], words - 1))
        refused("library_offsets", lambda: _bad_offsets(S, parsed, pod_node, words))
        if S.device_count() >= 2 or getattr(S, "_SIM_ACTIVE", False):
            other = S.open_whatifs(parsed, pod_node, [[0]], device=1, derive=False)
            try:
                S.upload_batch(other, device=1)
                S.solve_batch_resident(other)
                refused("two_devices", lambda: S.command_rows([flats[0], other[0]], [0, 1], [0, 0], [1.0, 1.0], [[], []], words))
            finally:
                for f in other:
                    f.close()
        else:
            out["two_devices"] = "one device"
        out["still_the_same"] = good().tobytes() == before
    finally:
        for f in flats:
            f.close()
        parsed.close()
    return out


def _bad_offsets(S, parsed, pod_node, words):
    import ctypes
    kh = S.libs()[1]
    off, cand = (ctypes.c_uint32 * 3)(0, 1, 0), (ctypes.c_uint32 * 2)(0, 0)
    pn = np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32))
    rows = np.zeros((2, S.command_row_words(words)), dtype=np.uint64)
    kh.ksh_consolidation_commands.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    rc = kh.ksh_consolidation_commands(parsed._p, 0, 2, off, cand, pn.ctypes.data, None, 0, 0, 0, rows.ctypes.data, words, None)
    if rc != S.KS_OK:
        raise S.KSolveError(rc, kh.ksh_last_error().decode())


SPECIAL = {"map_miss": map_miss_run, "mixed_t": mixed_t_run, "refusals": refusals_run}

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_consolidation_commands as T
out = {}
for name in jobs["names"]:
    try:
        out[name] = T.SPECIAL[name](S) if name in T.SPECIAL else T.device_run(S, name)
    except Exception as e:
        import traceback
        out[name] = {"error": repr(e)[:300] + traceback.format_exc()[-1500:]}
print("RESULT " + json.dumps(out))
"""


def run_in_child(names, sim, tmp):
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    path = os.path.join(tmp, f"jobs_{len(os.listdir(tmp))}.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "names": names}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in names}
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return run_in_child(CASES + list(SPECIAL), True, str(tmp_path_factory.mktemp("commands_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return run_in_child(CASES + list(SPECIAL), bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("commands_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


# ---------------------------------------------------------------------------------------------------------------- the reference
_REF = {}


def ref_decision(name, i, same_type):
    """What oracle/consolidation_ref.py says of candidate set i of a case: {action, reason, narrowed, command (canonical) or "error", requirements of new node 0,
    options of both stages as type names}.  The action, options and requirements are CR.compute_consolidation's / CR.filter_out_same_type's own; the reason is read
    off the same simulation with CR's predicates, in the reference's order."""
    key = (name, i, same_type)
    if key in _REF:
        return _REF[key]
    snap, sets, _ = case(name)
    cs = sets[i]
    types = {it.name: it for it in snap.instance_types}
    out = {"narrowed": False, "options": [], "options2": [], "node_reqs": None, "n_new": None}
    if set(cs) & set(snap.deleting):
        out.update(action=ERROR, reason=WHY_DELETING, command="error")
        _REF[key] = out
        return out
    sink = []
    try:
        cmd = CR.compute_consolidation(snap, cs, sink)
    except ValueError:
        cmd = None
    res = sink[0]
    out["n_new"], out["n_unscheduled"] = len(res.new_nodes), len(res.unscheduled)
    if res.new_nodes:
        out["node_reqs"] = CR.canon_reqs(dict(res.new_nodes[0].requirements))
    gone = set(cs) | set(snap.deleting)
    blocked = any(n.in_state and n.owned and n.labels.get("karpenter.sh/initialized") != "true" for j, n in enumerate(snap.nodes) if j not in gone)
    if cmd is None:
        assert not blocked and not res.unscheduled and len(res.new_nodes) == 1
        out.update(action=ERROR, reason=WHY_PRICE_ERROR, command="error")
    elif cmd[0] == "delete":
        out.update(action=DELETE, reason=0, command=list(CR.canonical(cmd)))
    elif cmd[0] == "do-nothing":
        if blocked or res.unscheduled:
            why = WHY_NOT_ALL_SCHEDULED
        elif len(res.new_nodes) != 1:
            why = WHY_MANY_NODES
        else:
            node = res.new_nodes[0]
            kept = CR.filter_by_price(types, node.instance_types, dict(node.requirements), CR.get_node_prices(types, [CR.Cand(snap, j) for j in cs]))
            why = WHY_NOT_CHEAPER if not kept else WHY_SPOT_TO_SPOT
            out["options"] = kept
        out.update(action=DO_NOTHING, reason=why, command=list(CR.canonical(cmd)))
    else:
        ct = res.new_nodes[0].requirements.get(CT)
        out.update(action=REPLACE, reason=0, command=list(CR.canonical(cmd)), options=list(cmd[2]), narrowed=CR.req_has(ct, "spot") and CR.req_has(ct, "on-demand"))
        out["node_reqs"] = CR.canon_reqs(cmd[3])
        if same_type:
            out["options2"] = CR.filter_out_same_type(snap, cmd[2], cmd[3], cs)
            if not out["options2"]:
                out.update(action=DO_NOTHING, reason=WHY_SAME_TYPE)
    _REF[key] = out
    return out


def _names(snap, idx):
    return [snap.instance_types[t].name for t in idx]


def _got(res, name):
    got = res[name]
    assert "error" not in got, got["error"]
    return got


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_rows_match_compute_consolidation(request, backend, name):
    """Every candidate set of every case: action, reason, narrowing, counts, both option stages, the decoded Command's canonical form and -- key by key -- the
    requirements the row carries, against the oracle's new node 0 (narrowed where the command is)."""
    got = _got(request.getfixturevalue(backend), name)
    snap, sets, _ = case(name)
    for tag, same in (("plain", False), ("same_type", True)):
        for i, cs in enumerate(sets):
            want, row = ref_decision(name, i, same), got[tag][i]
            # the narrowed bit belongs to a replace; a replace that step 9 turned down (do-nothing, KS_CMD_WHY_SAME_TYPE) keeps it (ksolve.h KS_CMD_DECISION)
            was_a_replace = want["action"] == REPLACE or want["reason"] == WHY_SAME_TYPE
            want_narrowed = want["narrowed"] and was_a_replace
            assert (row["action"], row["reason"], row["narrowed"]) == (want["action"], want["reason"], want_narrowed), (tag, cs, row, want)
            assert row["id"] == i
            if want["reason"] == WHY_DELETING:
                continue
            assert (row["n_new"], row["n_unscheduled"]) == (want["n_new"], want["n_unscheduled"]), (tag, cs)
            assert sorted(_names(snap, row["options"])) == sorted(want["options"]) and row["n_options"] == len(want["options"]), (tag, cs, row, want)
            assert sorted(_names(snap, row["options_same_type"])) == sorted(want["options2"]) and row["n_options_same_type"] == len(want["options2"]), (tag, cs, row, want)
            if want["node_reqs"] is not None:
                have = {k: (v[0], tuple(v[1]), v[2], v[3]) for k, v in row["requirements"].items()}
                assert sorted(have) == sorted(want["node_reqs"]), (tag, cs)
                for k in have:
                    assert have[k] == want["node_reqs"][k], (tag, cs, k, have[k], want["node_reqs"][k])
            else:
                assert row["requirements"] == {}
            if not same:
                assert json.loads(json.dumps(got["plain_cmd"][i])) == json.loads(json.dumps(want["command"])), (cs, got["plain_cmd"][i], want["command"])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("price-")])
def test_searches_match_the_reference(request, backend, name):
    """ksh_first_n_node_option and ksh_single_node_option against CR.first_n_node_consolidation_option / CR.single_node_consolidation_option (the binary search
    returns the probed prefix's error)."""
    got = _got(request.getfixturevalue(backend), name)
    snap, _, multi = case(name)
    try:
        want = json.loads(json.dumps(list(CR.first_n_node_consolidation_option(snap, multi))))
    except ValueError:
        want = "error"
    assert json.loads(json.dumps(got["first_n"])) == want
    want_single = json.loads(json.dumps(list(CR.single_node_consolidation_option(snap, multi))))
    assert json.loads(json.dumps(got["single"])) == want_single
    if "py_single" in got:       # consolidation.py's own route, a second opinion: a difference here is a finding about existing code
        assert json.loads(json.dumps(got["py_first_n"])) == want and json.loads(json.dumps(got["py_single"])) == want_single


@pytest.mark.parametrize("backend", BACKENDS)
def test_volume_snapshot_takes_the_fallback_and_the_flags(request, backend):
    """A snapshot with CSI volume limits and claims: ksh_open_whatifs_derived refuses it without KSH_DERIVE_VOLUMES, so the plain call (checked against the oracle by
    test_rows_match_compute_consolidation) ran the fallback -- what-ifs flattened one by one and uploaded --; with KSH_DERIVE_VOLUMES the what-ifs are derived, with
    KSH_ACTIVE_RESOURCES the snapshot is flattened over the active names: the same rows, byte for byte, every time."""
    got = _got(request.getfixturevalue(backend), "volumes")
    assert got["derivation_refused_without_flag"] and got["derived_with_flag"]
    for tag in ("derive_volumes", "active_resources", "both_flags"):
        assert got[tag + "_hex"] == got["same_type_hex"], tag
    assert len({(r["action"], r["reason"]) for r in got["plain"]}) >= 2          # (not one answer for every set)


def test_the_row_layout_constants_are_the_headers():
    """scheduler.KS_CMD_* and this file's own copies against the #defines of include/ksolve.h."""
    import re
    from karpenter_core_amd import scheduler as S
    text = open(os.path.join(ROOT, "include", "ksolve.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (KS_CMD_[A-Z_]+) (\d+)u?\b", text)}
    assert len(defs) >= 25
    for name, value in defs.items():
        if name != "KS_CMD_F_ALL":
            assert getattr(S, name) == value, name
    assert (DO_NOTHING, DELETE, REPLACE, ERROR) == (defs["KS_CMD_DO_NOTHING"], defs["KS_CMD_DELETE"], defs["KS_CMD_REPLACE"], defs["KS_CMD_ERROR"])
    assert (WHY_NOT_ALL_SCHEDULED, WHY_MANY_NODES, WHY_PRICE_ERROR, WHY_NOT_CHEAPER, WHY_SPOT_TO_SPOT, WHY_SAME_TYPE, WHY_DELETING) == tuple(
        defs["KS_CMD_WHY_" + n] for n in ("NOT_ALL_SCHEDULED", "MANY_NODES", "PRICE_ERROR", "NOT_CHEAPER", "SPOT_TO_SPOT", "SAME_TYPE", "DELETING"))
    assert (F_BLOCKED, F_ALL_SPOT, F_PRICE_ERROR, F_SAME_TYPE) == tuple(defs["KS_CMD_F_" + n] for n in ("BLOCKED", "ALL_SPOT", "PRICE_ERROR", "SAME_TYPE"))
    assert S.command_row_words(3) == defs["KS_CMD_OPTIONS"] + 6 and defs["KS_CMD_OPTIONS"] == 72 == defs["KS_CMD_BOUNDS"] + 32 and defs["KS_CMD_BOUNDS"] == defs["KS_CMD_MASK"] + 32


def test_every_branch_is_reached_by_the_cases():
    """(CPU, the oracle alone) Over the committed cases every reason code and every action occurs, filterOutSameType both keeps and empties, a command is narrowed to
    spot and one is not.  Zero branches uncovered."""
    reasons, actions, narrowed, stage2 = set(), set(), set(), set()
    for name in CASES:
        for i in range(len(case(name)[1])):
            for same in (False, True):
                d = ref_decision(name, i, same)
                reasons.add(d["reason"]); actions.add(d["action"])
                if d["action"] == REPLACE:
                    narrowed.add(d["narrowed"])
                    if same:
                        stage2.add("kept")
                if d["reason"] == WHY_SAME_TYPE:
                    stage2.add("emptied")
    assert reasons == {0, WHY_NOT_ALL_SCHEDULED, WHY_MANY_NODES, WHY_PRICE_ERROR, WHY_NOT_CHEAPER, WHY_SPOT_TO_SPOT, WHY_SAME_TYPE, WHY_DELETING}, reasons
    assert actions == {DO_NOTHING, DELETE, REPLACE, ERROR}
    assert narrowed == {True, False} and stage2 == {"kept", "emptied"}


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_go_map_miss_prices_a_listed_type_at_zero(request, backend):
    """A candidate type none of whose candidates has an offering is listed at 0.0; where stage 1 kept that type the second ceiling is 0.0 and nothing passes a strict <.
    The reference: CR.filter_out_same_type over the same snapshot, whose candidate has no offering."""
    got = _got(request.getfixturevalue(backend), "map_miss")
    snap, _ = TC._missing_offering()
    assert [p for _, p in got["listed"]] == [0.0]
    sink = []
    with pytest.raises(ValueError):
        CR.compute_consolidation(snap, [0], sink)
    node = sink[0].new_nodes[0]
    types = {it.name: it for it in snap.instance_types}
    kept = CR.filter_by_price(types, node.instance_types, dict(node.requirements), CR.MAX_FLOAT64)
    assert snap.nodes[0].labels[LABEL_INSTANCE_TYPE] in kept                      # the listed type is among the kept options: its 0.0 is the ceiling
    assert sorted(_names(snap, got["row"]["options"])) == sorted(kept)
    assert CR.filter_out_same_type(snap, kept, dict(node.requirements), [0]) == [] == got["row"]["options_same_type"]
    assert (got["row"]["action"], got["row"]["reason"]) == (DO_NOTHING, WHY_SAME_TYPE)
    # without the listed type the ceiling is MaxFloat64: what stage 1 kept is priced again under the (narrowed) requirements against that
    reqs = dict(node.requirements)
    if CR.req_has(reqs.get(CT), "spot") and CR.req_has(reqs.get(CT), "on-demand"):
        reqs[CT] = CR.Narrowed(["spot"])
    again = CR.filter_by_price(types, kept, reqs, CR.MAX_FLOAT64)
    assert again and sorted(_names(snap, got["unlisted"]["options_same_type"])) == sorted(again) and got["unlisted"]["action"] == REPLACE


@pytest.mark.parametrize("backend", BACKENDS)
def test_price_edges_are_strict(request, backend):
    """Candidates priced exactly at a worst launch price lose the types at that price, one ulp above keeps them (checked against the oracle above; here: that the
    cases contain both sides and that they differ), with 64 zone x capacity-type pairs, T = 65 and T > 4096."""
    res = request.getfixturevalue(backend)
    on_edge = above = 0
    for name in PRICE:
        got = _got(res, name)
        snap, sets, _ = case(name)
        types = {it.name: it for it in snap.instance_types}
        for i, cs in enumerate(sets):
            price = CR.get_node_prices(types, [CR.Cand(snap, cs[0])])
            sink = []
            CR.compute_consolidation(snap, cs, sink)
            if len(sink[0].new_nodes) != 1:
                continue
            node = sink[0].new_nodes[0]
            worst = {n: CR.worst_launch_price(types[n].offerings, dict(node.requirements)) for n in node.instance_types}
            kept = set(_names(snap, got["plain"][i]["options"]))
            for n, w in worst.items():
                if w == price:
                    assert n not in kept
                    on_edge += 1
                if math.nextafter(w, math.inf) == price:
                    assert n in kept
                    above += 1
    assert on_edge >= 10 and above >= 10
    assert len(case("price-types_65-41")[0].instance_types) == 65 and len(case("price-tw_over_64-51")[0].instance_types) > 4096
    zs = {o.zone for it in case("price-pairs_64-37")[0].instance_types for o in it.offerings}
    assert len(zs) * 2 == 64


@pytest.mark.parametrize("backend", BACKENDS)
def test_one_call_over_what_ifs_of_different_t(request, backend):
    got = _got(request.getfixturevalue(backend), "mixed_t")
    assert len(set(got["words"])) > 1
    res = request.getfixturevalue(backend)
    for k, name in enumerate(MIXED):
        own = _got(res, name)["plain"]
        for i, row in enumerate(got["rows"][k]):
            assert row["id"] == k * 1000 + i
            assert {x: row[x] for x in row if x != "id"} == {x: own[i][x] for x in own[i] if x != "id"}, (name, i)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_row_hygiene(request, backend, name):
    """A poisoned buffer, rows three words wider than the catalogue needs, ids shuffled, the call made twice: no poison word survives, the tails are zero, rows come
    back in the order of the ids given, the second call returns the same bytes -- and the rows are those of ksh_consolidation_commands."""
    got = _got(request.getfixturevalue(backend), name)
    h = got["hygiene"]
    assert h["poison_left"] == 0 and h["tails_zero"] and h["same_bytes"] and h["ids"] == h["want_ids"]
    snap, sets, _ = case(name)
    words = (len(snap.instance_types) + 63) // 64
    for k, i in enumerate(h["live_in_order"]):
        whole = got["same_type_hex"][i]
        assert h["narrow"][k] == whole[: 2 * 8 * (72 + 2 * words)], (name, i)


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(request, backend):
    """KS_ERR_INVALID with a message for: a row narrower than the catalogue, a type index >= T, offsets that do not ascend, an unknown flag
    bit (the kernel's and the library's), a batch over two devices; afterwards the same handles answer as before.  (A problem without prices cannot be made through
    libkshost: tests/cabi_usage_commands.c strips them from a flat problem.)"""
    got = _got(request.getfixturevalue(backend), "refusals")
    for tag, needle in (("words_short", "too short"), ("type_index", "type index"), ("offsets", "ascending"), ("flag_bit", "flag bit"),
                        ("library_flag_bit", "flag bit"), ("library_words_short", "too short"), ("library_offsets", "ascending")):
        assert got[tag][0] == -1 and needle in got[tag][1], (tag, got[tag])
    if got["two_devices"] != "one device":
        assert got["two_devices"][0] == -1 and "devices" in got["two_devices"][1]
    else:
        assert backend == "gpu"          # one device on this box: this leg has NOT made the two-device call; the emulator leg always makes it
    assert got["still_the_same"]


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_commands")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_commands.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    snap, cands, _ = TC.scenarios()["can_replace_node"]
    from karpenter_core_amd import workloads as W
    pr, pod_node = W.snapshot_problem(snap.instance_types, snap.provisioner, snap.nodes, snap.bound)
    f = tmp_path / "snapshot.ksp"
    f.write_text(pr.to_ksp())
    out = subprocess.run([exe, str(f)] + [str(int(x)) for x in pod_node], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    want = CR.compute_consolidation(snap, cands)
    assert f"command 0: replace remove n1 options {len(want[2])}:" in out.stdout, out.stdout
    line = [l for l in out.stdout.splitlines() if l.startswith("command 0:")][0]
    assert sorted(line.split("options ")[1].split(": ")[1].split(" | ")[0].split()) == sorted(want[2])
    for k, v in CR.canon_reqs(want[3]).items():
        assert f"{k} {'NotIn' if v[0] else 'In'} [{' '.join(v[1])}]" in line, (k, v, line)
    assert "single node option: replace remove n1" in out.stdout
    assert "refused without prices: problem carries no offering prices" in out.stdout


def test_c_abi_from_c_on_the_emulator(tmp_path):
    """tests/cabi_usage_commands.c -- snapshot in, commands printed -- as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries."""
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_c_abi_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
