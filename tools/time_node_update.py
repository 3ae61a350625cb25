#!/usr/bin/env python3
"""What one node reconciliation costs the snapshot (kshost.h NODE=, state.Cluster.UpdateNode) -- host only, no GPU needed.
   usage: tools/time_node_update.py [nodes] [reps]
   On `cluster_snapshot(nodes)` one node's initialised label flips, three ways, median of `reps`:
     (a) one NODE= event, the flattening continued;
     (b) what expressed the same change before the event existed: NODE-, NODE+, then a BIND for every pod the node ran (a new slot, the pods appended again);
     (c) the snapshot ingested again (parse + flattening from scratch).
   The library's own time for events + flattening (`apply`'s "ms"); (c) is the parse and the flattening timed around the calls."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses
import numpy as np
from karpenter_core_amd import scheduler as S, workloads as W
args = [a for a in sys.argv[1:] if not a.startswith("--")]
nn = int(args[0]) if len(args) > 0 else 2048
reps = int(args[1]) if len(args) > 1 else 9
INIT = "karpenter.sh/initialized"
its, prov, nodes, bound = W.cluster_snapshot(nn, 50, 45)
nodes[1].labels[INIT] = "false"      # (both values are in the cluster throughout)
snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
text = snap.to_ksp().encode()
update, rebind, ingest = [], [], []
a, b = S.ParsedProblem.from_text(text), S.ParsedProblem.from_text(text)
a.snapshot_fingerprint(pn); b.snapshot_fingerprint(pn)
rs = np.random.RandomState(3)
cur, cur_b, first = nodes, bound, True
for r in range(reps):
    i = 2 + r      # a node that is in its original slot in both snapshots
    flipped = dataclasses.replace(cur[i], labels=dict(cur[i].labels, **{INIT: "false" if cur[i].labels[INIT] == "true" else "true"}))
    info = a.apply_block([("node=", flipped)], pn if first else None)
    assert info["continued"], info
    update.append(info["ms"])
    # (b): the node leaves and joins again with the label flipped; `available` as a node without pods has it, the BINDs take the requests off again
    empty = W.cluster_after(cur, cur_b, [("unbind", p.uid) for p in cur_b[i]])[0][i]
    ev = [("node-", cur[i].name), ("node+", dataclasses.replace(empty, labels=flipped.labels))] + [("bind", cur[i].name, p) for p in cur_b[i]]
    info = b.apply_block(ev, pn if first else None)
    assert info["continued"], info
    rebind.append(info["ms"])
    first = False
    t = time.perf_counter()
    c = S.ParsedProblem.from_text(text); c.snapshot_fingerprint(pn)
    ingest.append((time.perf_counter() - t) * 1e3)
    c.close()
med = statistics.median
print(f"{nn} nodes / {len(pn)} pods, median of {reps} (min .. max), {os.cpu_count()} host threads visible")
print(f"  one NODE= event, continued                      {med(update):8.2f} ms  ({min(update):.2f} .. {max(update):.2f})")
print(f"  NODE-, NODE+, BIND x pods of the node, continued {med(rebind):8.2f} ms  ({min(rebind):.2f} .. {max(rebind):.2f})")
print(f"  the snapshot ingested again (parse + flatten)   {med(ingest):8.2f} ms  ({min(ingest):.2f} .. {max(ingest):.2f})")
a.close(); b.close()
