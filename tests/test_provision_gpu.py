"""Provisioner.Reconcile's scheduling pass over the snapshot kept by events (include/kshost.h ksh_provision / ksh_placement_rows; kernels ks_placement_heads /
ks_placement_rows in csrc/ksolve.hip; provisioning/provisioner.go:106-165).  Every batch shape must give the same placement rows (pod, node slot / new node j / -1,
relaxation stage, reason, commit order per node), machine rows and launch picks by three roads: ksh_provision, oracle_py.solve over the equivalent Problem, and
ksh_solve_from_batch over the same objects (compared by uid).  As in tests/test_replacement_commands.py every case runs unmarked on the emulator in a child process and
marked `gpu` on the device; the comparisons happen here."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import workloads as W
from karpenter_core_amd.model import (Container, DO_NOT_SCHEDULE, Expr, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME, LABEL_ZONE, LabelSelector, Pod, PodAffinityTerm, PreferredTerm,
                                      StateNode, TopologySpreadConstraint)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POISON = 0xA5A5A5A5A5A5A5A5
CARRIER = "~pending~"
NODES = 24


# ---------------------------------------------------------------------------------------------------------------- the clusters
def _pending(n, seed, prefix="pending"):
    rs = np.random.RandomState(seed)
    return [W.generic_pod(rs, f"{prefix}-{i:04d}") for i in range(n)]


def _small(uid, cpu="10m", mem="10Mi"):
    return Pod(uid=uid, labels={"my-label": "a"}, containers=[Container(requests={"cpu": cpu, "memory": mem})])


def _with_topology(nodes, bound):
    """Bound pods of workloads a, b, c carry terms: a spreads over zones, b over hostnames, c refuses its own kind per hostname (moved to nodes of its own first)."""
    seen_c = set()
    for e, pods in enumerate(bound):
        for p in pods:
            lab = p.labels["my-label"]
            own = LabelSelector({"my-label": lab})
            if lab == "a":
                p.spread = [TopologySpreadConstraint(3, LABEL_ZONE, DO_NOT_SCHEDULE, own)]
            elif lab == "b":
                p.spread = [TopologySpreadConstraint(4, LABEL_HOSTNAME, DO_NOT_SCHEDULE, own)]
            elif lab == "c":
                if e in seen_c:
                    p.labels = {"my-label": "d"}      # (at most one per node: the anti-affinity holds in the snapshot)
                else:
                    seen_c.add(e)
                    p.anti_required = [PodAffinityTerm(LABEL_HOSTNAME, own)]


_BUILT = {}


def case(name):
    """-> dict(its, prov, nodes, bound, pending, deleting, group_lists, events): `nodes` / `bound` without the carrier; `deleting` the nodes marked for deletion."""
    if name in _BUILT:
        return _BUILT[name]
    c = {"group_lists": False, "events": False, "deleting": []}
    if name == "volumes_fallback":
        its, prov, nodes, bound = W.volume_snapshot(NODES, 5, 8, unowned=False)
    else:
        its, prov, nodes, bound = W.cluster_snapshot(NODES, 5, 8)
    if name in ("p1", "p70", "p300"):
        pending = _pending(int(name[1:]), 100 + int(name[1:]))
    elif name == "all_existing":
        pending = [_small(f"tiny-{i}") for i in range(5)]
    elif name == "two_machines":
        pending = [_small(f"big-{i:02d}", "3", "2Gi") for i in range(40)]
    elif name == "unschedulable":
        pending = _pending(3, 7) + [_small(f"huge-{i}", "4000", "1Gi") for i in range(2)]
    elif name == "relaxes":
        pending = _pending(3, 9)
        for i in range(2):
            p = _small(f"picky-{i}", "100m", "100Mi")
            p.preferred_affinity = [PreferredTerm(10, [Expr(LABEL_ZONE, "In", ["no-such-zone"])])]
            pending.append(p)
    elif name == "deleting2":
        pending, c["deleting"] = _pending(10, 11), [9, 19]
    elif name in ("topology", "topology_lists"):
        _with_topology(nodes, bound)
        pending = [dataclasses.replace(p, uid=f"more-{e}-{k}") for e in range(8, 12) for k, p in enumerate(bound[e][:3])] + _pending(6, 13)
        c["deleting"], c["group_lists"] = [10], name == "topology_lists"
    elif name == "volumes_fallback":
        pending, c["deleting"] = _pending(8, 15), [8]
    elif name == "after_events":
        pending, c["events"] = _pending(20, 17), True
    else:
        raise KeyError(name)
    c.update(its=its, prov=prov, nodes=nodes, bound=bound, pending=pending)
    _BUILT[name] = c
    return c


CASES = ["p1", "p70", "p300", "all_existing", "two_machines", "unschedulable", "relaxes", "deleting2", "topology", "topology_lists", "volumes_fallback", "after_events"]


def snapshot_of(c, pending=None):
    """(snapshot Problem, pod_node, leaving): every node a state node plus the carrier (last slot), the pending pods bound to it; the carrier's pods are not cluster pods."""
    pending = c["pending"] if pending is None else pending
    nodes, bound = list(c["nodes"]) + [StateNode(name=CARRIER)], list(c["bound"]) + [list(pending)]
    snap, pod_node = W.snapshot_problem(c["its"], c["prov"], nodes, bound)
    snap.cluster_pods = [cp for cp in snap.cluster_pods if cp.node_name != CARRIER]
    return snap, pod_node, [len(nodes) - 1] + list(c["deleting"])


def problem_of(c):
    """The equivalent Problem: Reconcile's Solve (provisioner.go:117-150) -- the pending pods, then the pods of the nodes marked for deletion, against the nodes that stay."""
    nodes, bound = list(c["nodes"]) + [StateNode(name=CARRIER)], list(c["bound"]) + [list(c["pending"])]
    pr = W.whatif(c["its"], c["prov"], nodes, bound, [len(nodes) - 1] + list(c["deleting"]))
    pr.cluster_pods = [cp for cp in pr.cluster_pods if cp.node_name != CARRIER]
    return pr


_REF = {}


def ref(name):
    """The oracle's Solve of the equivalent Problem, by uid: what every road must say."""
    if name not in _REF:
        from oracle import oracle_py as O
        c = case(name)
        pr = problem_of(c)
        res = O.solve(pr)
        uid = [p.uid for p in pr.pods]
        canon = res.canonical()
        _REF[name] = {"new": [[uid[i] for i in n.pods] for n in res.new_nodes], "existing": {k: [uid[i] for i in v] for k, v in res.existing.items() if v},
                      "unscheduled": [uid[i] for i in res.unscheduled], "stage": {uid[i]: s for i, s in enumerate(res.final_stage)},
                      "reasons": {uid[i]: r for i, r in res.reasons.items()},
                      "machines": [{"options": sorted(n.instance_types), "requirements": norm(m["requirements"]), "requests": m["requests"]} for n, m in zip(res.new_nodes, canon["new_nodes"])],
                      "picks": [literal_pick(c["its"], n) for n in res.new_nodes], "n_pods": len(pr.pods)}
    return _REF[name]


def literal_pick(its, node):
    """fake/cloudprovider.go:79-84 over the node's options: the type whose cheapest available offering compatible with the node's zone / capacity-type requirements is
    cheapest, ties to the lowest catalogue index -> [type name, price] or None."""
    def has(key, v):
        r = node.requirements.get(key)
        return True if r is None else ((v in r.values) != r.complement)
    best = None
    for t, it in enumerate(its):
        if it.name not in node.instance_types:
            continue
        prices = [o.price for o in it.offerings if o.available and has(LABEL_ZONE, o.zone) and has(LABEL_CAPACITY_TYPE, o.capacity_type)]
        if prices and (best is None or min(prices) < best[1]):
            best = [it.name, min(prices)]
    return best


def norm(x):
    return json.loads(json.dumps(x))


# ---------------------------------------------------------------------------------------------------------------- the device side
def _decode_tables(S, snap, parsed, got, words):
    head = got["head"]
    uid = [p.uid for p in snap.pods]
    rows = [S.decode_placement_row(r, head["n_existing"]) for r in got["rows"]] if got["rows"] is not None else None
    out = {"route": got["route"], "head": head, "total_rows": got["total_rows"], "total_machines": got["total_machines"], "ms": got["ms"], "rows": rows}
    if rows is not None:
        ls = S.placement_lists(rows)
        out["lists"] = {"new": [[uid[i] for i in ls["new"].get(j, [])] for j in range(head["n_new"])], "existing": {snap.nodes[s].name: [uid[i] for i in v] for s, v in ls["existing"].items()},
                        "unscheduled": [uid[i] for i in ls["unscheduled"]], "stage": {uid[i]: s for i, s in ls["stage"].items()}, "reasons": {uid[i]: r for i, r in ls["reasons"].items()}}
        out["positions"] = [d["position"] for d in rows]
        out["ids"] = sorted({d["id"] for d in rows})
        out["pods"] = [d["pod"] for d in rows]
    if got["machines"] is not None:
        ms = []
        for row in got["machines"]:
            d = S.decode_replacement_node(parsed, row, words)
            ms.append({"options": sorted(snap.instance_types[t].name for t in d["options"]), "requirements": d["requirements"], "requests": d["requests"], "node": d["node"]})
        out["machines"] = ms
    if got["picks"] is not None:
        import ctypes
        kh = S.libs()[1]
        kh.ksh_snapshot_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        kh.ksh_snapshot_name.restype = ctypes.c_char_p
        out["picks"] = [None if p is None else [snap.instance_types[p[0]].name, kh.ksh_snapshot_name(parsed._p, 5, p[1], 0).decode(), kh.ksh_snapshot_name(parsed._p, 6, p[2], 0).decode(), p[3]]
                        for p in got["picks"]]
    return out


def _third_road(S, c):
    """ksh_solve_from_batch over the same objects: the environment without pods, the batch through the binary door; by uid, with the launch picks off its handle."""
    from karpenter_core_amd.model import pods_to_blocks
    pr = problem_of(c)
    env = S.ParsedProblem(dataclasses.replace(pr, pods=[]))
    batch = S.PodBatch(pods_to_blocks(pr.pods))
    fp, _ = S.solve_from_batch(env, batch)
    try:
        res = fp.result()
        uid = [p.uid for p in pr.pods]
        picks = S.launch_pick([fp] * len(res.new_nodes), list(range(len(res.new_nodes))))
        return {"machines": [{"options": sorted(n.instance_types), "requirements": m["requirements"], "requests": m["requests"]} for n, m in zip(res.new_nodes, res.canonical()["new_nodes"])],
                "new": [[uid[i] for i in n.pods] for n in res.new_nodes], "existing": {k: [uid[i] for i in v] for k, v in res.existing.items() if v},
                "unscheduled": [uid[i] for i in res.unscheduled], "stage": {uid[i]: s for i, s in enumerate(res.final_stage)}, "reasons": {uid[i]: r for i, r in res.reasons.items()},
                "picks": [None if p is None else [c["its"][p[0]].name, p[1], p[2], p[3]] for p in picks]}
    finally:
        fp.close(); batch.close(); env.close()


def device_run(S, name):
    if name == "handles":
        return handles_run(S)
    if name == "refusals":
        return refusals_run(S)
    if name == "ordinary":
        return ordinary_run(S)
    if name == "mirror":
        return mirror_run(S)
    if name == "dev_tables":
        return dev_tables_run(S)
    c = case(name)
    words = (len(c["its"]) + 63) // 64
    snap, pod_node, leaving = snapshot_of(c)
    fl = S.KSH_DERIVE_GROUP_LISTS if c["group_lists"] else 0
    out = {}
    if c["events"]:      # the pending pods arrive as BIND events to the (empty) carrier; the library holds the bindings from then on
        snap0, pod_node0, _ = snapshot_of(c, pending=[])
        parsed = S.ParsedProblem(snap0)
        info = parsed.apply_block([("bind", CARRIER, p) for p in c["pending"]], pod_node0)
        out["applied"] = info["applied"]
        before = S.whatifs_simulated()
        got = S.provision(parsed, None, leaving, words, flags=fl)
        out["simulated"] = S.whatifs_simulated() - before
        out["patched"] = _decode_tables(S, snap, parsed, got, words)
        parsed.close()
    parsed = S.ParsedProblem(snap)
    try:
        before = S.whatifs_simulated()
        got = S.provision(parsed, pod_node, leaving, words, flags=fl)
        out.setdefault("simulated", S.whatifs_simulated() - before)
        out["fresh"] = _decode_tables(S, snap, parsed, got, words)
        P, M = got["total_rows"], got["total_machines"]
        # the sizing call: nothing but the head and the totals
        z = S.provision(parsed, pod_node, leaving, words, cap_rows=0, cap_machines=0, flags=fl)
        out["sizing"] = {"head": z["head"], "total_rows": z["total_rows"], "total_machines": z["total_machines"], "rows": z["rows"] is None, "machines": z["machines"] is None}
        # hygiene: poisoned tables two rows longer, machine rows two words wider; every word of every row written, reserved words zero, nothing beyond touched
        rp = np.full((P + 2, S.KS_PLC_ROW_WORDS), POISON, dtype=np.uint64)
        mp = np.full((M + 2, S.replacement_node_words(words + 2)), POISON, dtype=np.uint64)
        h = S.provision(parsed, pod_node, leaving, words + 2, cap_rows=P + 2, cap_machines=M + 2, flags=fl, rows=rp, machines=mp)
        base = S.KS_REP_NODE_OPTIONS
        out["hygiene"] = {"rows_equal": bool((rp[:P] == got["rows"]).all()), "no_poison": bool((rp[:P] != POISON).all()) and bool((mp[:M] != POISON).all()),
                          "beyond_intact": bool((rp[P:] == POISON).all()) and bool((mp[M:] == POISON).all()), "head_equal": h["head"] == got["head"],
                          "machines_equal": bool((mp[:M, :base + words] == got["machines"]).all()) if M else True, "surplus_zero": bool((mp[:M, base + words:] == 0).all())}
        # one row short, one machine short
        rs_, ms_ = np.full((P + 1, S.KS_PLC_ROW_WORDS), POISON, dtype=np.uint64), np.full((M + 1, S.replacement_node_words(words)), POISON, dtype=np.uint64)
        s = S.provision(parsed, pod_node, leaving, words, cap_rows=P - 1, cap_machines=max(M - 1, 0), flags=fl, rows=rs_, machines=ms_)
        out["short"] = {"head": s["head"], "total_rows": s["total_rows"], "total_machines": s["total_machines"], "rows_intact": bool((rs_ == POISON).all()),
                        "machines_intact": bool((ms_ == POISON).all()) if M else True, "rows": s["rows"] is None, "machines": s["machines"] is None, "picks": s["picks"] is None}
    finally:
        parsed.close()
    out["batch"] = _third_road(S, c)
    return norm(json.loads(json.dumps(out, default=lambda o: o.tolist() if hasattr(o, "tolist") else list(o))))


def _arrays_view(fp):
    ra = fp.result_arrays()
    off = ra["node_pods_off"]
    return {"n_existing": ra["n_existing"], "n_new": ra["n_new"], "pod_node": ra["pod_node"].tolist(), "pod_stage": ra["pod_stage"].tolist(), "pod_reason": ra["pod_reason"].tolist(),
            "unscheduled": ra["unscheduled"].tolist(), "node_pods": [ra["node_pods"][off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]}


def ordinary_run(S):
    """ksh_placement_rows over handles that are NO what-ifs over a snapshot: a Solve through the binary door (ksh_solve_from_batch), one from the pod list
    (ksh_solve_from_pods) and one flattened from objects already held (ksh_open_parsed) -- all three flattened over the environment cache --, and a plain ksh_open handle;
    beside each the arrays ksh_result_arrays_get gives."""
    import ctypes
    from karpenter_core_amd.model import pods_to_blocks
    kh = S.libs()[1]
    prs = [problem_of(case(n)) for n in ("two_machines", "unschedulable", "relaxes", "deleting2")]
    keep, flats = [], []
    try:
        env = S.ParsedProblem(dataclasses.replace(prs[0], pods=[])); batch = S.PodBatch(pods_to_blocks(prs[0].pods)); keep += [env, batch]
        flats.append(S.solve_from_batch(env, batch)[0])
        held = S.ParsedProblem(prs[1]); keep.append(held)
        flats.append(S.solve_from_pods(held)[0])
        held2 = S.ParsedProblem(prs[2]); keep.append(held2)
        h = ctypes.c_void_p()
        kh.ksh_open_parsed.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
        assert kh.ksh_open_parsed(held2._p, 0, ctypes.byref(h)) == S.KS_OK, kh.ksh_last_error()
        flats.append(S.FlatProblem(None, _handle=h)); flats[-1].upload(0); flats[-1].solve(decode=False)
        flats.append(S.FlatProblem(prs[3])); flats[-1].upload(0); flats[-1].solve(decode=False)
        heads, rows, total = S.placement_rows(flats, [3, 4, 5, 6])
        return norm({"heads": [S.decode_placement_head(x) for x in heads], "rows": rows.tolist(), "total": total, "arrays": [_arrays_view(f) for f in flats],
                     "E": [sum(1 for n in pr.nodes if n.in_state) for pr in prs], "P": [len(pr.pods) for pr in prs]})
    finally:
        for f in flats:
            f.close()
        for k in keep:
            k.close()


def _snapshot_dataclass(c):
    from karpenter_core_amd import consolidation as C
    return C.Snapshot(c["its"], c["prov"], list(c["nodes"]), [list(b) for b in c["bound"]], list(c["pending"]), tuple(c["deleting"]))


def mirror_run(S):
    """consolidation.provision_dev: the shapes Solve returns, as names and uids."""
    from karpenter_core_amd import consolidation as C
    out = {}
    for name in ("two_machines", "deleting2", "unschedulable", "relaxes", "nothing"):
        c = dict(case("p1"), pending=[]) if name == "nothing" else case(name)
        timings = {}
        got = C.provision_dev(_snapshot_dataclass(c), C.CandidateInfo(node_age_seconds=[0.0] * NODES), timings=timings)
        out[name] = {"route": got.route, "nodes": [{"provisioner": n.ProvisionerName, "pods": [p.uid for p in n.Pods], "options": sorted(it.name for it in n.InstanceTypeOptions),
                                                    "requirements": {k: [r.complement, sorted(r.values), r.greater_than, r.less_than] for k, r in n.Requirements.items()},
                                                    "requests": dict(n.Requests)} for n in got.nodes],
                     "existing": {e.Node.name: [p.uid for p in e.Pods] for e in got.existing}, "unscheduled": [[p.uid, r] for p, r in got.unscheduled], "stages": got.stages,
                     "picks": [None if p is None else [p[0], p[3]] for p in got.picks], "timed": sorted(timings)}
    return norm(out)


def dev_tables_run(S):
    """ks_placement_rows_dev into the CALLER's device tables (hipMalloc'ed here; the emulator's device memory is the host's): the same heads and rows as
    ks_placement_rows_host over the same problems, nothing beyond the rows written; a row table that is not 32-byte aligned is refused with nothing written."""
    import ctypes
    ks, kh = S.libs()
    sim = bool(getattr(S, "_SIM_ACTIVE", False))
    fps = [S.FlatProblem(problem_of(case(n))) for n in ("two_machines", "unschedulable")]
    kh.ksh_problem.restype = ctypes.c_void_p
    kh.ksh_problem.argtypes = [ctypes.c_void_p]
    ks.ks_problem_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    ks.ks_problem_free.argtypes = [ctypes.c_void_p]
    ks.ks_solve_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    ks.ks_placement_rows_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    ks.ks_placement_rows_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    ds, owned = (ctypes.c_void_p * 2)(), []
    try:
        for i, fp in enumerate(fps):
            d = ctypes.c_void_p()
            assert ks.ks_problem_upload(kh.ksh_problem(fp._h), 0, ctypes.byref(d)) == S.KS_OK, ks.ks_last_error()
            ds[i] = d.value
            one = (ctypes.c_void_p * 1)(d.value)
            assert ks.ks_solve_batch_dev(one, 1, None, None) == S.KS_OK, ks.ks_last_error()      # (no result buffers: the results stay on the device)
        ids, total = np.asarray([11, 12], dtype=np.uint64), ctypes.c_uint64(0)
        P = sum(f.dims["P"] for f in fps)
        hh, hr = np.zeros((2, S.KS_PLC_HEAD_WORDS), dtype=np.uint64), np.zeros((P, S.KS_PLC_ROW_WORDS), dtype=np.uint64)
        assert ks.ks_placement_rows_host(ds, 2, ids.ctypes.data, hh.ctypes.data, hr.ctypes.data, P, ctypes.byref(total), None) == S.KS_OK, ks.ks_last_error()
        words = (P + 2) * S.KS_PLC_ROW_WORDS + 4      # two rows of room beyond the table, and room to start it at a 32-byte boundary
        if sim:
            raw = np.full(words, POISON, dtype=np.uint64)
            dh = np.full(2 * S.KS_PLC_HEAD_WORDS, POISON, dtype=np.uint64)
            rows_ptr, heads_ptr = raw.ctypes.data, dh.ctypes.data
            back = lambda: (raw.copy(), dh.copy())
        else:      # device memory of the caller's own, from the HIP runtime the library is linked against
            hip = ctypes.CDLL("libamdhip64.so")
            hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
            hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
            hip.hipFree.argtypes = [ctypes.c_void_p]
            raw, dh = np.full(words, POISON, dtype=np.uint64), np.full(2 * S.KS_PLC_HEAD_WORDS, POISON, dtype=np.uint64)
            d_raw, d_dh = ctypes.c_void_p(), ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(d_raw), raw.nbytes) == 0 and hip.hipMalloc(ctypes.byref(d_dh), dh.nbytes) == 0
            owned += [(hip, d_raw), (hip, d_dh)]
            assert hip.hipMemcpy(d_raw, raw.ctypes.data, raw.nbytes, 1) == 0 and hip.hipMemcpy(d_dh, dh.ctypes.data, dh.nbytes, 1) == 0      # (1: host to device)
            rows_ptr, heads_ptr = d_raw.value, d_dh.value

            def back():
                a, b = np.zeros_like(raw), np.zeros_like(dh)
                assert hip.hipMemcpy(a.ctypes.data, d_raw, a.nbytes, 2) == 0 and hip.hipMemcpy(b.ctypes.data, d_dh, b.nbytes, 2) == 0      # (2: device to host)
                return a, b
        skip = ((-rows_ptr) % 32) // 8      # words to the first 32-byte boundary
        t2 = ctypes.c_uint64(0)
        rc_mis = ks.ks_placement_rows_dev(ds, 2, ids.ctypes.data, heads_ptr, rows_ptr + 8 * skip + 8, P, ctypes.byref(t2))
        msg_mis = ks.ks_last_error().decode()
        r0, h0 = back()
        rc = ks.ks_placement_rows_dev(ds, 2, ids.ctypes.data, heads_ptr, rows_ptr + 8 * skip, P, ctypes.byref(t2))
        r1, h1 = back()
        tab = r1[skip:skip + P * S.KS_PLC_ROW_WORDS].reshape(P, S.KS_PLC_ROW_WORDS)
        return norm({"misaligned": [rc_mis, msg_mis, bool((r0 == POISON).all()) and bool((h0 == POISON).all())], "rc": rc, "total": [int(total.value), int(t2.value), P],
                     "heads_equal": bool((h1.reshape(2, -1) == hh).all()), "rows_equal": bool((tab == hr).all()), "rows_nonzero": bool(hr.any()),
                     "around_intact": bool((r1[:skip] == POISON).all()) and bool((r1[skip + P * S.KS_PLC_ROW_WORDS:] == POISON).all())})
    finally:
        for hip, ptr in owned:
            hip.hipFree(ptr)
        for d in ds:
            if d:
                ks.ks_problem_free(d)
        for f in fps:
            f.close()


def handles_run(S):
    """ksh_placement_rows over three what-ifs of different sizes, one of them empty, on both routes; its ids; the table one row short."""
    c = case("deleting2")
    snap, pod_node, leaving = snapshot_of(c)
    carrier = leaving[0]
    sets = [[carrier], [], list(leaving)]
    parsed = S.ParsedProblem(snap)
    out = {"sets": sets, "n_pods": [sum(1 for n in pod_node if n in cs) for cs in sets]}
    try:
        for route, derive in (("derived", True), ("flattened", False)):
            flats = S.open_whatifs(parsed, pod_node, sets, derive=derive, device=0)
            try:
                if not derive:
                    S.upload_batch(flats, 0)
                S.solve_batch_resident(flats)
                heads, rows, total = S.placement_rows(flats, [7, 8, 9])
                hp, rp = np.full((3, S.KS_PLC_HEAD_WORDS), POISON, dtype=np.uint64), np.full((total + 1, S.KS_PLC_ROW_WORDS), POISON, dtype=np.uint64)
                h2, _, t2 = S.placement_rows(flats, [7, 8, 9], cap_rows=total - 1, heads=hp, rows=rp)
                d2 = [S.decode_placement_head(h) for h in h2]
                written = d2[0]["pods"]
                out[route] = {"heads": [S.decode_placement_head(h) for h in heads], "rows": rows.tolist() if rows is not None else [], "total": total,
                              "arena": [f.arena_bytes() for f in flats],
                              "short": {"total": t2, "truncated": [d["truncated"] for d in d2], "row_off": [d["row_off"] for d in d2], "no_head_poison": bool((hp != POISON).all()),
                                        "below_identical": bool((rp[:written] == rows[:written]).all()), "beyond_intact": bool((rp[written:] == POISON).all())}}
            finally:
                for f in flats:
                    f.close()
    finally:
        parsed.close()
    return norm(out)


def refusals_run(S):
    """Every refusal: codes and messages, and that nothing was written."""
    import ctypes
    ks, kh = S.libs()
    c = case("p1")
    words = (len(c["its"]) + 63) // 64
    snap, pod_node, leaving = snapshot_of(c)
    parsed = S.ParsedProblem(snap)
    out = {}

    def refused(tag, fn):
        try:
            fn()
            out[tag] = None
        except S.KSolveError as e:
            out[tag] = [e.code, str(e)]
    try:
        refused("unknown_flag", lambda: S.provision(parsed, pod_node, leaving, words, flags=1 << 30))
        refused("deleting_out_of_range", lambda: S.provision(parsed, pod_node, [len(snap.nodes)], words))
        refused("no_bindings", lambda: S.provision(parsed, None, leaving, words, cap_rows=4, cap_machines=4))
        # straight at the C ABI: NULL out, a capacity with a NULL table, pick arrays given in part
        kh.ksh_provision.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        pn, dl = np.asarray(pod_node, dtype=np.int32), np.asarray(leaving, dtype=np.uint32)
        out["null_out"] = kh.ksh_provision(parsed._p, 0, pn.ctypes.data, dl.ctypes.data, len(leaving), 0, None, None)
        po = S._ProvisionOut()
        po.words, po.cap_rows = words, 4
        out["null_table"] = kh.ksh_provision(parsed._p, 0, pn.ctypes.data, dl.ctypes.data, len(leaving), 0, ctypes.byref(po), None)
        po = S._ProvisionOut()
        ty = np.zeros(4, dtype=np.int32)
        po.words, po.pick_type = words, ty.ctypes.data
        out["partial_picks"] = kh.ksh_provision(parsed._p, 0, pn.ctypes.data, dl.ctypes.data, len(leaving), 0, ctypes.byref(po), None)
        po = S._ProvisionOut()
        po.words = words - 1      # one option word fewer than the catalogue needs
        out["row_too_short"] = [kh.ksh_provision(parsed._p, 0, pn.ctypes.data, dl.ctypes.data, len(leaving), 0, ctypes.byref(po), None), kh.ksh_last_error().decode()]
        out["null_deleting"] = kh.ksh_provision(parsed._p, 0, pn.ctypes.data, None, 1, 0, ctypes.byref(S._ProvisionOut()), None)
        # nothing pending and nothing on a deleting node: zero rows, no what-if, every lap zero
        before = S.whatifs_simulated()
        e = S.provision(parsed, pod_node, [], words, cap_rows=4, cap_machines=4)
        e2 = S.provision(parsed, pod_node, [3], words, cap_rows=0, cap_machines=0) if not c["bound"][3] else None
        out["empty"] = {"route": e["route"], "total_rows": e["total_rows"], "total_machines": e["total_machines"], "head": e["head"], "ms": e["ms"], "simulated": S.whatifs_simulated() - before,
                        "rows": len(e["rows"]), "empty_node_too": e2 is None or e2["route"] == "nothing"}
        # ksh_placement_rows: a handle that was opened but not solved; NULL ids; ksh_result_arrays_get still refuses a derived handle
        flats = S.open_whatifs(parsed, pod_node, [[leaving[0]]], derive=True, device=0)
        try:
            refused("rows_before_solve", lambda: S.placement_rows(flats, [0], cap_rows=8))
            kh.ksh_placement_rows.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
            hs = (ctypes.c_void_p * 1)(flats[0]._h)
            heads, total = np.zeros(S.KS_PLC_HEAD_WORDS, dtype=np.uint64), ctypes.c_uint64(0)
            S.solve_batch(flats)
            out["rows_null_ids"] = kh.ksh_placement_rows(hs, 1, None, heads.ctypes.data, None, 0, ctypes.byref(total), None)
            out["rows_null_total"] = kh.ksh_placement_rows(hs, 1, heads.ctypes.data, heads.ctypes.data, None, 0, None, None)
            out["rows_null_table"] = kh.ksh_placement_rows(hs, 1, heads.ctypes.data, heads.ctypes.data, None, 4, ctypes.byref(total), None)
            refused("result_arrays_of_derived", lambda: flats[0].result_arrays())
        finally:
            for f in flats:
                f.close()
        # the device half: a problem that was uploaded and never solved, NULL arrays
        fp = S.FlatProblem(problem_of(c))
        try:
            kh.ksh_problem.restype = ctypes.c_void_p
            kh.ksh_problem.argtypes = [ctypes.c_void_p]
            ks.ks_problem_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
            ks.ks_problem_free.argtypes = [ctypes.c_void_p]
            ks.ks_placement_rows_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
            ks.ks_placement_rows_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
            d = ctypes.c_void_p()
            assert ks.ks_problem_upload(kh.ksh_problem(fp._h), 0, ctypes.byref(d)) == S.KS_OK
            ds = (ctypes.c_void_p * 1)(d)
            ids, heads, total = np.zeros(1, dtype=np.uint64), np.full(S.KS_PLC_HEAD_WORDS, POISON, dtype=np.uint64), ctypes.c_uint64(5)
            out["dev_never_solved"] = [ks.ks_placement_rows_host(ds, 1, ids.ctypes.data, heads.ctypes.data, None, 0, ctypes.byref(total), None), ks.ks_last_error().decode(), int(total.value)]
            out["dev_null_ds"] = ks.ks_placement_rows_host(None, 1, ids.ctypes.data, heads.ctypes.data, None, 0, ctypes.byref(total), None)
            out["dev_null_ids"] = ks.ks_placement_rows_host(ds, 1, None, heads.ctypes.data, None, 0, ctypes.byref(total), None)
            out["dev_null_heads"] = ks.ks_placement_rows_host(ds, 1, ids.ctypes.data, None, None, 0, ctypes.byref(total), None)
            out["dev_null_member"] = ks.ks_placement_rows_host((ctypes.c_void_p * 1)(None), 1, ids.ctypes.data, heads.ctypes.data, None, 0, ctypes.byref(total), None)
            out["dev_null_total"] = ks.ks_placement_rows_dev(ds, 1, ids.ctypes.data, heads.ctypes.data, None, 0, None)
            out["dev_null_rows"] = ks.ks_placement_rows_dev(ds, 1, ids.ctypes.data, heads.ctypes.data, None, 4, ctypes.byref(total))
            out["dev_heads_untouched"] = bool((heads == POISON).all())
            ks.ks_problem_free(d)
        finally:
            fp.close()
    finally:
        parsed.close()
    return norm(out)


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_provision_gpu as T
out = {}
for name in jobs["names"]:
    try:
        out[name] = T.device_run(S, name)
    except Exception as e:
        import traceback
        out[name] = {"error": repr(e)[:300] + traceback.format_exc()[-1500:]}
print("RESULT " + json.dumps(out))
"""


def run_in_child(names, sim, tmp):
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    path = os.path.join(tmp, "jobs.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "names": names}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in names}
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return run_in_child(CASES + ["handles", "refusals", "ordinary", "mirror", "dev_tables"], True, str(tmp_path_factory.mktemp("provision_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return run_in_child(CASES + ["handles", "refusals", "ordinary", "mirror", "dev_tables"], bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("provision_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


def _got(res, name):
    got = res[name]
    assert "error" not in got, got["error"]
    return got


def _same_as_ref(tables, want, where):
    ls = tables["lists"]
    assert ls["new"] == want["new"], (where, "Node.Pods in commit order")
    assert ls["existing"] == want["existing"], (where, "ExistingNode.Pods in commit order")
    assert ls["unscheduled"] == want["unscheduled"], (where, "the queue as Solve left it")
    assert ls["stage"] == want["stage"], (where, "relaxation stages")
    assert ls["reasons"] == norm(want["reasons"]), (where, "reasons")
    assert tables["positions"] == list(range(want["n_pods"])) and tables["ids"] == ([0] if want["n_pods"] else []), where
    assert len(set(tables["pods"])) == want["n_pods"], where
    h = tables["head"]
    assert (h["id"], h["pods"], h["n_new"], h["n_unscheduled"], h["row_off"], h["truncated"], h["machines_truncated"], h["reserved"]) == \
           (0, want["n_pods"], len(want["new"]), len(want["unscheduled"]), 0, False, False, 0), (where, h)
    assert h["n_existing"] == NODES + 1 and tables["total_rows"] == want["n_pods"] and tables["total_machines"] == len(want["new"]), (where, h)
    assert len(tables["machines"]) == len(want["machines"])
    for j, (g, w) in enumerate(zip(tables["machines"], want["machines"])):
        assert g["node"] == j and g["options"] == w["options"], (where, j)
        assert g["requirements"] == w["requirements"], (where, j, g["requirements"], w["requirements"])
        assert g["requests"] == w["requests"], (where, j)
    assert [None if p is None else [p[0], p[3]] for p in tables["picks"]] == norm(want["picks"]), (where, "launch picks")


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_three_roads_agree(request, backend, name):
    """ksh_provision == the oracle == ksh_solve_from_batch, by uid: Node.Pods and ExistingNode.Pods in commit order, the unscheduled queue, every pod's relaxation stage
    and reason word, the machines (options, requirements, requests) and the launch picks (zone and capacity type against the pick off the batch road's handle)."""
    got, want = _got(request.getfixturevalue(backend), name), ref(name)
    _same_as_ref(got["fresh"], want, (name, "fresh"))
    b = got["batch"]
    for k in ("new", "existing", "unscheduled", "stage"):
        assert b[k] == want[k], (name, "ksh_solve_from_batch", k)
    assert b["reasons"] == norm(want["reasons"])
    assert got["fresh"]["picks"] == b["picks"], name
    assert b["machines"] == want["machines"] and [{k: m[k] for k in ("options", "requirements", "requests")} for m in got["fresh"]["machines"]] == b["machines"], (name, "machines by the batch road")
    assert got["simulated"] == 1
    assert got["fresh"]["route"] == ("flattened" if name == "volumes_fallback" else "derived"), got["fresh"]["route"]
    ms = got["fresh"]["ms"]
    assert ms["open_ms"] > 0.0 and ms["solve_ms"] > 0.0 and ms["command_kernel_ms"] > 0.0 and ms["readback_ms"] > 0.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_after_bind_events_patched_equals_fresh_equals_the_oracle(request, backend):
    """The pending pods bound to the carrier by ksh_env_apply_block, the bindings held by the library (pod_node NULL): the same tables, word for word, as over a snapshot
    ingested with them, and the oracle's."""
    got, want = _got(request.getfixturevalue(backend), "after_events"), ref("after_events")
    assert got["applied"] == 20
    _same_as_ref(got["patched"], want, "patched")
    for k in ("rows", "machines", "picks", "head"):
        assert got["patched"][k] == got["fresh"][k], k


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_sizing_capacity_and_hygiene(request, backend, name):
    """The sizing call gives heads and totals only.  Poisoned, longer and wider tables: every word of every row written, surplus words zero, nothing beyond the rows
    touched.  One row and one machine short: KS_OK with the full totals, both truncated flags, and not one word of either table written."""
    got, want = _got(request.getfixturevalue(backend), name), ref(name)
    P, M = want["n_pods"], len(want["new"])
    z = got["sizing"]
    assert (z["total_rows"], z["total_machines"], z["rows"], z["machines"]) == (P, M, True, M > 0), z
    assert z["head"] == dict(got["fresh"]["head"], truncated=True, machines_truncated=M > 0)
    assert all(got["hygiene"].values()), got["hygiene"]
    s = got["short"]
    assert (s["total_rows"], s["total_machines"]) == (P, M) and s["head"] == z["head"] and s["rows"] and s["rows_intact"] and s["machines_intact"], s
    assert s["machines"] == (M > 0) and s["picks"] == (M > 0)


def test_the_cases_say_what_they_should():
    """CPU: the oracle's own answers on the cases whose point is a particular shape."""
    assert ref("p1")["n_pods"] == 1 and ref("p70")["n_pods"] == 70 and ref("p300")["n_pods"] == 300
    a = ref("all_existing")
    assert not a["new"] and not a["unscheduled"] and sum(len(v) for v in a["existing"].values()) == 5
    assert len(ref("two_machines")["new"]) >= 2 and len(ref("p300")["new"]) >= 2
    u = ref("unschedulable")
    assert sorted(u["unscheduled"]) == ["huge-0", "huge-1"] and all(u["reasons"][p] != 0 for p in u["unscheduled"])
    r = ref("relaxes")
    assert r["stage"]["picky-0"] > 0 and r["stage"]["picky-1"] > 0 and not r["unscheduled"]
    d = case("deleting2")
    assert ref("deleting2")["n_pods"] == 10 + len(d["bound"][9]) + len(d["bound"][19]) and len(d["bound"][9]) and len(d["bound"][19])
    assert "node-00009" not in ref("deleting2")["existing"] and "node-00019" not in ref("deleting2")["existing"]
    t = case("topology")
    assert any(p.spread for p in t["pending"]) and any(p.anti_required for p in t["pending"]) and any(p.anti_required for b in t["bound"] for p in b)
    assert ref("topology") == ref("topology_lists")
    v = case("volumes_fallback")
    assert any(n.volume_limits for n in v["nodes"]) and any(p.volumes for b in v["bound"] for p in b)
    # pods on existing nodes, on new ones and left over all occur somewhere, and some node takes more than one pod (commit order is exercised)
    assert any(len(v) > 1 for n in CASES for v in ref(n)["new"]) and any(len(v) > 1 for n in CASES for v in ref(n)["existing"].values())


@pytest.mark.parametrize("backend", BACKENDS)
def test_placement_rows_over_open_handles(request, backend):
    """ksh_placement_rows over three what-ifs of different sizes, the middle one empty: its own ids, row_off as the exclusive sum in what-if order, every what-if's rows
    the oracle's; the derived route and the flattened route give the SAME tables word for word (snapshot pod indices, node slots); one row short the last what-if is
    truncated, the first one's rows are written and nothing beyond them is."""
    from oracle import oracle_py as O
    got = _got(request.getfixturevalue(backend), "handles")
    c = case("deleting2")
    snap, pod_node, leaving = snapshot_of(c)
    from karpenter_core_amd import scheduler as S
    d, f = got["derived"], got["flattened"]
    assert all(a > 0 for a in d["arena"]) and not any(f["arena"])
    assert d["heads"] == f["heads"] and d["rows"] == f["rows"] and d["total"] == f["total"] == sum(got["n_pods"])
    offs = np.cumsum([0] + got["n_pods"])
    uid = [p.uid for p in snap.pods]
    for i, (cs, h) in enumerate(zip(got["sets"], d["heads"])):
        assert (h["id"], h["pods"], h["row_off"], h["truncated"], h["n_existing"]) == (7 + i, got["n_pods"][i], int(offs[i]), False, NODES + 1), h
        rows = [S.decode_placement_row(r, h["n_existing"]) for r in d["rows"][h["row_off"]:h["row_off"] + h["pods"]]]
        assert all(r["id"] == 7 + i for r in rows) and [r["position"] for r in rows] == list(range(h["pods"]))
        pr = W.whatif(c["its"], c["prov"], snap.nodes, list(c["bound"]) + [list(c["pending"])], cs)
        pr.cluster_pods = [cp for cp in pr.cluster_pods if cp.node_name != CARRIER]
        res = O.solve(pr)
        wuid = [p.uid for p in pr.pods]
        ls = S.placement_lists(rows)
        assert (h["n_new"], h["n_unscheduled"]) == (len(res.new_nodes), len(res.unscheduled))
        assert [[uid[p] for p in ls["new"].get(j, [])] for j in range(h["n_new"])] == [[wuid[p] for p in n.pods] for n in res.new_nodes], i
        assert {snap.nodes[s].name: [uid[p] for p in v] for s, v in ls["existing"].items()} == {k: [wuid[p] for p in v] for k, v in res.existing.items() if v}, i
        assert {uid[p]: s for p, s in ls["stage"].items()} == {wuid[p]: s for p, s in enumerate(res.final_stage)}
    for r in (d, f):
        s = r["short"]
        assert s["total"] == d["total"] and s["truncated"] == [False, False, True] and s["row_off"] == [int(x) for x in offs[:-1]]
        assert s["no_head_poison"] and s["below_identical"] and s["beyond_intact"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_placement_rows_over_handles_that_are_no_whatifs(request, backend):
    """A Solve through ksh_solve_from_batch, ksh_solve_from_pods or ksh_open_parsed is flattened over the environment cache and shares an Encoded, like a what-if over a
    snapshot -- and is none: its rows keep the handle's OWN pod indices and existing-node indices (E unrenamed), word for word what ksh_result_arrays_get says: where
    every pod went, its stage, its reason word, and per node the pods in ascending commit number."""
    from karpenter_core_amd import scheduler as S
    got = _got(request.getfixturevalue(backend), "ordinary")
    off = 0
    assert got["total"] == sum(got["P"])
    for i, (h, a) in enumerate(zip(got["heads"], got["arrays"])):
        assert (h["id"], h["pods"], h["row_off"], h["truncated"], h["n_existing"], h["n_new"], h["n_unscheduled"]) == \
               (3 + i, got["P"][i], off, False, got["E"][i], a["n_new"], len(a["unscheduled"])), (i, h)
        assert a["n_existing"] == got["E"][i]
        rows = [S.decode_placement_row(r, h["n_existing"]) for r in got["rows"][off:off + h["pods"]]]
        off += h["pods"]
        assert sorted(r["pod"] for r in rows) == list(range(h["pods"])) and [r["position"] for r in rows] == list(range(h["pods"])) and all(r["id"] == 3 + i for r in rows)
        for r in rows:
            assert (r["where"], r["stage"], r["reason"]) == (a["pod_node"][r["pod"]], a["pod_stage"][r["pod"]], a["pod_reason"][r["pod"]]), (i, r)
            assert (r["seq"] < 0) == (r["where"] < 0)
        assert [r["pod"] for r in rows if r["where"] < 0] == a["unscheduled"]
        by_node = {}
        for r in sorted((r for r in rows if r["where"] >= 0), key=lambda r: r["seq"]):
            by_node.setdefault(r["where"], []).append(r["pod"])
        assert [by_node.get(n, []) for n in range(len(a["node_pods"]))] == a["node_pods"], i
    assert any(a["n_new"] for a in got["arrays"]) and any(a["unscheduled"] for a in got["arrays"]) and any(s > 0 for a in got["arrays"] for s in a["pod_stage"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_provision_dev_returns_what_solve_returns(request, backend):
    """consolidation.provision_dev against the oracle: Node.Pods in commit order with options, requirements and requests, ExistingNode.Pods, the unscheduled pods with
    their reason words, the stages to apply back, the picks; an empty pass simulates nothing."""
    got = _got(request.getfixturevalue(backend), "mirror")
    for name in ("two_machines", "deleting2", "unschedulable", "relaxes"):
        g, want = got[name], ref(name)
        assert g["route"] == "derived" and g["timed"] == ["command_kernel_ms", "host_ms", "open_ms", "readback_ms", "solve_ms"]
        assert [n["pods"] for n in g["nodes"]] == want["new"] and all(n["provisioner"] == "default" for n in g["nodes"]), name
        assert [{k: n[k] for k in ("options", "requirements", "requests")} for n in g["nodes"]] == want["machines"], name
        assert g["existing"] == want["existing"], name
        assert g["unscheduled"] == [[u, want["reasons"][u]] for u in want["unscheduled"]], name
        assert g["stages"] == {u: s for u, s in want["stage"].items() if s > 0}, name
        assert g["picks"] == norm(want["picks"]), name
    assert got["nothing"] == {"route": "nothing", "nodes": [], "existing": {}, "unscheduled": [], "stages": {}, "picks": [], "timed": got["nothing"]["timed"]}


@pytest.mark.parametrize("backend", BACKENDS)
def test_rows_into_the_callers_device_tables(request, backend):
    """ks_placement_rows_dev: heads and rows in the caller's own device buffers equal the host twin's, the words around the table stay as they were; a row table off the
    32-byte boundary is KS_ERR_INVALID with neither table touched.  (A batch over two devices cannot be made on one GPU: that refusal is BatchStage::open's, shared with
    every call over a batch and tested where two devices exist.)"""
    from karpenter_core_amd import scheduler as S
    d = _got(request.getfixturevalue(backend), "dev_tables")
    assert d["misaligned"][0] == S.KS_ERR_INVALID and "32-byte aligned" in d["misaligned"][1] and d["misaligned"][2], d["misaligned"]
    assert d["rc"] == S.KS_OK and d["total"][0] == d["total"][1] == d["total"][2]
    assert d["heads_equal"] and d["rows_equal"] and d["rows_nonzero"] and d["around_intact"], d


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals(request, backend):
    """Every refusal, on both halves of the ABI, with nothing written; the empty pass; ksh_result_arrays_get's refusal of a derived handle stays."""
    from karpenter_core_amd import scheduler as S
    r = _got(request.getfixturevalue(backend), "refusals")
    assert r["unknown_flag"][0] == S.KS_ERR_INVALID and "unknown flag bit" in r["unknown_flag"][1]
    assert r["row_too_short"][0] == S.KS_ERR_INVALID and "row too short" in r["row_too_short"][1]
    assert r["deleting_out_of_range"][0] == S.KS_ERR_INVALID and "out of range" in r["deleting_out_of_range"][1]
    assert r["no_bindings"][0] == S.KS_ERR_INVALID and "bindings" in r["no_bindings"][1]
    for k in ("null_out", "null_table", "partial_picks", "null_deleting", "rows_null_ids", "rows_null_total", "rows_null_table"):
        assert r[k] == S.KS_ERR_INVALID, k
    assert r["rows_before_solve"][0] == S.KS_ERR_INVALID and "before solve" in r["rows_before_solve"][1]
    assert r["result_arrays_of_derived"][0] == S.KS_ERR_UNSUPPORTED
    e = r["empty"]
    assert (e["route"], e["total_rows"], e["total_machines"], e["simulated"], e["rows"]) == ("nothing", 0, 0, 0, 0) and e["empty_node_too"]
    assert all(v == 0 for v in e["head"].values()) and all(v == 0.0 for v in e["ms"].values())
    assert r["dev_never_solved"][0] == S.KS_ERR_INVALID and "holds no result" in r["dev_never_solved"][1] and r["dev_never_solved"][2] == 0
    for k in ("dev_null_ds", "dev_null_ids", "dev_null_heads", "dev_null_member", "dev_null_total", "dev_null_rows"):
        assert r[k] == S.KS_ERR_INVALID, k
    assert r["dev_heads_untouched"]


# ---------------------------------------------------------------------------------------------------------------- the C ABI from C
def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_provision")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_provision.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    c = case("deleting2")
    snap, pod_node, leaving = snapshot_of(c)
    f = tmp_path / "snapshot.ksp"
    f.write_text(snap.to_ksp())
    out = subprocess.run([exe, str(f), str(leaving[0]), str(leaving[1]), str(leaving[2])] + [str(int(x)) for x in pod_node], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    want = ref("deleting2")
    assert f"sizing: {want['n_pods']} rows, {len(want['new'])} machines" in lines, out.stdout
    assert f"head: {want['n_pods']} pods, {len(want['new'])} new, {len(want['unscheduled'])} unscheduled, route 1" in lines, out.stdout
    uid = [p.uid for p in snap.pods]
    placed = {}
    for l in lines:
        if l.startswith("pod "):
            _, pod, _, where, _, stage = l.split()
            placed[uid[int(pod)]] = (int(where), int(stage))
    slot = {n.name: i for i, n in enumerate(snap.nodes)}
    expect = {u: (slot[k], want["stage"][u]) for k, v in want["existing"].items() for u in v}
    expect.update({u: (len(snap.nodes) + j, want["stage"][u]) for j, v in enumerate(want["new"]) for u in v})
    expect.update({u: (-1, want["stage"][u]) for u in want["unscheduled"]})
    assert placed == expect
    assert sum(l.startswith("machine ") for l in lines) == len(want["new"]) and "refused: " in out.stdout


def test_c_abi_from_c_on_the_emulator(tmp_path):
    """tests/cabi_usage_provision.c as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries."""
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_c_abi_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
