"""Timing of derived consolidation what-ifs over the topology snapshot of tools/time_topology_whatifs.py (2 048 nodes, 512 what-ifs, bound pods with spread /
affinity / anti-affinity terms): the per-node facts behind a what-if's topology as dense tables (flag off) against lists per node (KSH_DERIVE_GROUP_LISTS).
Nine warm batches each: median with min and max of the open (host + upload + derivation kernels) and of the whole batch end to end (open, solve, records), and
the bytes one open copies to the device (ksh_whatifs_upload_bytes: the same in every batch).  Runs on a tree without the flag too (then only the dense leg).
    python tools/time_whatif_group_lists.py [NODES] [WHATIFS] [--lists | --dense]     (default: both legs, where the tree has the flag)
--apps=N: instead, the cluster of tests/test_whatif_group_lists.py at NODES nodes -- N two-pod applications, each with groups of its own (5 groups per 4 applications:
819 give the 1 024 groups the dense tables stop at) -- where the dense tables are as large as they get: 2 x G x NODES int32 per open."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from karpenter_core_amd import scheduler as S, workloads as W      # noqa: E402
from test_whatif_derived import _topology_snapshot                  # noqa: E402  (the generator of the differential tests)

args = [a for a in sys.argv[1:] if not a.startswith("--")]
nodes_n = int(args[0]) if len(args) > 0 else 2048
n_whatifs = int(args[1]) if len(args) > 1 else 512
has_flag = hasattr(S, "KSH_DERIVE_GROUP_LISTS")
legs = [l for l in ("dense", "lists") if ("--" + l in sys.argv or not any(a in sys.argv for a in ("--dense", "--lists"))) and (l == "dense" or has_flag)]
if any(a.startswith("--apps=") and int(a.split("=")[1]) * 5 // 4 > 1024 for a in sys.argv):
    legs = [l for l in legs if l == "lists"]      # (above the cap only the lists derive)
REPS = 9


def one(parsed, pod_node, sets, words, leg):
    kw = {"group_lists": True} if leg == "lists" else {}
    t0 = time.perf_counter()
    flats = S.open_whatifs(parsed, pod_node, sets, derive=True, **kw)
    t1 = time.perf_counter()
    up = flats[0].upload_bytes() if hasattr(flats[0], "upload_bytes") else None      # (a tree before the flag has no such accessor: its route is the flag-off one of a tree that has)
    S.solve_batch(flats, decode=False)
    rec = S.result_records(flats, list(range(len(sets))), words)
    t2 = time.perf_counter()
    for f in flats:
        f.close()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, rec, up


def spread(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "min": round(xs[0], 3), "max": round(xs[-1], 3)}


def main():
    apps = [int(a.split("=")[1]) for a in sys.argv if a.startswith("--apps=")]
    if apps:
        from test_whatif_group_lists import many_groups_cluster
        its, prov, nodes, bound, snap, pod_node = many_groups_cluster(apps[0], nodes_n)
    else:
        its, prov, nodes, bound, snap, pod_node = _topology_snapshot(nodes_n, 50, 45, spare=-1, extras=True, anti=True)
    sets = W.config4_sets(n_whatifs, nodes_n, 45)
    words = (len(its) + 63) // 64
    out = {"nodes": len(nodes), "bound_pods": len(snap.pods), "whatifs": len(sets), "groups": S.FlatProblem(snap).dims["G"], "reps": REPS}
    recs = {}
    for leg in legs:
        parsed = S.ParsedProblem(snap)
        _, first, recs[leg], up = one(parsed, pod_node, sets, words, leg)      # (the snapshot is flattened, made resident and its tables built here, once)
        runs = [one(parsed, pod_node, sets, words, leg)[:2] for _ in range(REPS)]
        out[leg] = {"first_batch_ms": round(first, 3), "open_ms": spread([r[0] for r in runs]), "end_to_end_ms": spread([r[1] for r in runs]), "upload_bytes": up}
        parsed.close()
    if len(recs) == 2:
        out["same_records"] = bool((recs["dense"] == recs["lists"]).all())
    print(json.dumps(out))


main()
