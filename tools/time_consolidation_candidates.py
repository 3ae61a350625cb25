#!/usr/bin/env python3
"""Times `ksh_consolidation_candidates` (candidateNodes + ShouldDeprovision + sortAndFilterCandidates on the device) at two shapes:
  config4    the config #4 snapshot (2 048 nodes and its bound pods) with 64 PDBs
  synthetic  100 000 pods / 4 096 nodes / 1 024 PDBs
Per shape: one untimed call, then the median of 9 with min - max, of the call's wall time and of the library's own split ms[0..3] (host tabulation, upload,
kernels, read-back).  Beside each, for orientation, the time of a single-thread literal host loop written here in Python (it measures the interpreter as much
as the work: an orientation, not a baseline) and whether it arrives at the same order.  No threshold: the numbers are a record.
--wide: at both shapes the narrow route and the wide-selector route (KSH_CAND_WIDE_SELECTORS) are timed interleaved, call by call, with the narrow / wide ratio of
kernels_ms and host_ms; and a third shape only the wide route accepts is added:
  per-app    the config #4 snapshot with one PDB per distinct `app` value (1 200 applications over 8 namespaces), every second PDB with disruptionsAllowed == 0"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import Expr, LabelSelector, Pod, PodDisruptionBudget, Problem, Provisioner, StateNode, pdbs_to_block


def med(xs):
    xs = sorted(xs)
    return f"{xs[len(xs) // 2]:9.3f} ms ({xs[0]:.3f} - {xs[-1]:.3f})"


def pdbs_for(n, keys, vals, rs):
    out = []
    for i in range(n):
        k = keys[int(rs.randint(len(keys)))]
        if i % 4 == 0:
            s = LabelSelector({}, [Expr(k, "NotIn", [vals[int(rs.randint(len(vals)))]]), Expr(keys[0], "Exists", [])])
        else:
            s = LabelSelector({k: vals[int(rs.randint(len(vals)))]}, [])
        out.append(PodDisruptionBudget(namespace=f"ns{int(rs.randint(8))}", selector=s, disruptions_allowed=int(i % 3 == 0)))
    return out


def host_loop(pods_ns, pods_labels, pod_node, pdbs, n_nodes, dc, age, ttl):
    """The literal single-thread loop, for orientation: per pod the first blocking PDB (pods x PDBs selector matches), per node the sequential sum."""
    t0 = time.perf_counter()
    by_ns = {}
    for i, b in enumerate(pdbs):
        if b.disruptions_allowed == 0:
            by_ns.setdefault(b.namespace, []).append((i, b.selector))
    cost, blocked = [0.0] * n_nodes, [-1] * n_nodes
    for p in range(len(pod_node)):
        nd = pod_node[p]
        c = 1.0 + dc[p] / 134217728.0
        cost[nd] += -10.0 if c < -10.0 else 10.0 if c > 10.0 else c
        if blocked[nd] < 0:
            lab = pods_labels[p]
            for i, s in by_ns.get(pods_ns[p], ()):
                ok = all(lab.get(k) == v for k, v in s.match_labels.items())
                for e in s.match_expressions:
                    if not ok:
                        break
                    ok = (e.key in lab) if e.op == "Exists" else not (e.key in lab and lab[e.key] in e.values)
                if ok:
                    blocked[nd] = i
                    break
    for n in range(n_nodes):
        cost[n] *= min(1.0, max(0.0, (ttl - age[n]) / ttl))
    order = sorted((n for n in range(n_nodes) if blocked[n] < 0), key=lambda n: cost[n])
    return (time.perf_counter() - t0) * 1e3, order


def run(tag, pr, pod_node, pdbs, rs, reps, routes=(False,)):
    """`routes`: the values of wide_selectors to time, interleaved call by call."""
    n_nodes, n_pods = len(pr.nodes), len(pr.pods)
    age = [float(x) for x in rs.uniform(0, 3000, n_nodes)]
    dc = [float(x) for x in rs.uniform(-1e9, 1e9, n_pods)]
    parsed = S.ParsedProblem(pr)
    block = pdbs_to_block(pdbs)
    kw = dict(node_flags=[0] * n_nodes, node_age_seconds=age, pod_flags=[S.KSH_CAND_POD_HAS_DELETION_COST] * n_pods, pod_deletion_cost=dc, pod_priority=[0] * n_pods,
              prov_consolidation_enabled=[True] * len(pr.provisioners), prov_ttl_seconds=[3600] * len(pr.provisioners), pdbs=block)
    got = {w: S.consolidation_candidates(parsed, pod_node, wide_selectors=w, **kw) for w in routes}          # untimed: first touch of the device, the label table
    wall, split = {w: [] for w in routes}, {w: {k: [] for k in S.CANDIDATE_TIMING_KEYS} for w in routes}
    for _ in range(reps):
        for w in routes:
            t0 = time.perf_counter()
            got[w] = S.consolidation_candidates(parsed, pod_node, wide_selectors=w, **kw)
            wall[w].append((time.perf_counter() - t0) * 1e3)
            for k in split[w]:
                split[w][k].append(got[w]["ms"][k])
    first = got[routes[0]]
    print(f"{tag}: {n_nodes} nodes, {n_pods} pods, {len(pdbs)} PDBs -> {len(first['order'])} candidates, {len(first['empty'])} empty")
    for w in routes:
        if len(routes) > 1 or w:
            print(f" {'wide' if w else 'narrow'} route")
        print(f"  call (Python wall, incl. array marshalling)  {med(wall[w])}")
        for k in S.CANDIDATE_TIMING_KEYS:
            print(f"  {k:<44} {med(split[w][k])}")
    if len(routes) > 1:
        same = all(got[w]["order"] == first["order"] and bytes(got[w]["cost"]) == bytes(first["cost"]) and list(got[w]["detail"]) == list(first["detail"]) for w in routes)
        mid = lambda w, k: sorted(split[w][k])[len(split[w][k]) // 2]
        print(f"  narrow / wide: kernels_ms {mid(False, 'kernels_ms') / mid(True, 'kernels_ms'):.2f}   host_ms {mid(False, 'host_ms') / mid(True, 'host_ms'):.2f}   same order, costs and details: {same}")
    hms, horder = host_loop([p.namespace for p in pr.pods], [p.labels for p in pr.pods], pod_node, pdbs, n_nodes, dc, age, 3600.0)
    print(f"  single-thread literal host loop (Python)     {hms:9.3f} ms   same order: {horder == first['order']}")
    parsed.close()


ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--skip-synthetic", action="store_true")
ap.add_argument("--wide", action="store_true", help="time the wide-selector route beside the narrow one, and the per-app shape only it accepts")
a = ap.parse_args()
rs = np.random.RandomState(12)
its, prov, nodes, bound = W.cluster_snapshot(2048, 50, 45)
keys4 = sorted({k for b in bound for p in b for k in p.labels}) or ["app"]
vals4 = sorted({v for b in bound for p in b for v in p.labels.values()})[:40] or ["x"]
for b in bound:
    for p in b:
        p.namespace = f"ns{int(rs.randint(8))}"
snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
for n in snap.nodes:
    n.labels.setdefault("karpenter.sh/initialized", "true")
routes = (False, True) if a.wide else (False,)
run("config4", snap, pod_node, pdbs_for(64, keys4[:6], vals4, rs), rs, a.reps, routes)
if not a.skip_synthetic:
    keys, vals = [f"key{i}" for i in range(8)], [f"val{i}" for i in range(40)]
    sn = [StateNode(name=f"n{i}", labels=dict(snap.nodes[0].labels)) for i in range(4096)]
    sp = [Pod(uid=f"p{i}", namespace=f"ns{int(rs.randint(8))}", labels={k: vals[int(rs.randint(40))] for k in keys if rs.rand() < 0.5}) for i in range(100000)]
    run("synthetic", Problem(instance_types=its, provisioners=[prov], pods=sp, nodes=sn, simulation_mode=True), [int(x) for x in rs.randint(0, 4096, 100000)], pdbs_for(1024, keys, vals, rs), rs, a.reps, routes)
if a.wide:      # one PDB per application: every pod gets an `app` of 1 200 and lives in its application's namespace
    for p in snap.pods:
        j = int(rs.randint(1200))
        p.labels["app"], p.namespace = f"app{j}", f"ns{j % 8}"
    apps = sorted({p.labels["app"] for p in snap.pods}, key=lambda s: int(s[3:]))
    per_app = [PodDisruptionBudget(namespace=f"ns{int(v[3:]) % 8}", selector=LabelSelector({"app": v}, []), disruptions_allowed=i % 2) for i, v in enumerate(apps)]
    assert len(per_app) >= 1000
    run("per-app", snap, pod_node, per_app, rs, a.reps, (True,))
