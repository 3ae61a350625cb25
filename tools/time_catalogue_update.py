#!/usr/bin/env python3
"""What one catalogue change costs the snapshot (kshost.h IT=, KSH_EVENT_INSTANCE_TYPE_UPDATE).
   usage: tools/time_catalogue_update.py [nodes] [reps] [--gpu]
   On `cluster_snapshot(nodes)` (2 048 nodes / 39 242 pods / 2 000 instance types by default) one offering's availability flips, two ways, median of `reps`, in the
   same run on the same host:
     (a) one IT= event, the flattening continued -- the library's own time for event + flattening (`apply`'s "ms");
     (b) the only road there was before the event existed: the snapshot ingested again with the new record (text written ahead of the clock; parse + flattening
         from scratch timed around the calls).
   --gpu: also the first batch of 512 what-ifs (workloads.config4_sets) after each -- opened (the snapshot's base made resident again), solved, records read --
   timed around the calls; needs a device.  KSH_TIMING=1 in the environment prints the flattening's phases to stderr."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dataclasses
from karpenter_core_amd import scheduler as S, workloads as W
args = [a for a in sys.argv[1:] if not a.startswith("--")]
gpu = "--gpu" in sys.argv
nn = int(args[0]) if len(args) > 0 else 2048
reps = int(args[1]) if len(args) > 1 else 9
its, prov, nodes, bound = W.cluster_snapshot(nn, 50, 45)
snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
sets = W.config4_sets(512, nn, 45)
words = (len(its) + 63) // 64


def first_batch(parsed, pod_node):
    t = time.perf_counter()
    flats = S.open_whatifs(parsed, pod_node, sets, derive=True)
    S.solve_batch(flats, decode=False)
    S.result_records(flats, list(range(len(flats))), words)
    ms = (time.perf_counter() - t) * 1e3
    for f in flats:
        f.close()
    return ms


a = S.ParsedProblem.from_text(snap.to_ksp().encode())
a.snapshot_fingerprint(pn)
if gpu:
    first_batch(a, pn)      # (resident before the first event, as in a pass that has run before)
update, ingest, after_update, after_ingest = [], [], [], []
cur = list(its)
for r in range(reps):
    t = 7 + 11 * r      # a type with several offerings; another one every time
    offs = [dataclasses.replace(o, available=(not o.available if j == 0 else o.available)) for j, o in enumerate(cur[t].offerings)]
    cur[t] = W.with_offerings(cur[t], offs)
    info = a.apply_block([("IT=", cur[t])], pn if r == 0 else None)
    assert info["continued"], info
    update.append(info["ms"])
    if gpu:
        after_update.append(first_batch(a, None))
    text = dataclasses.replace(snap, instance_types=cur).to_ksp().encode()
    t0 = time.perf_counter()
    c = S.ParsedProblem.from_text(text); c.snapshot_fingerprint(pn)
    ingest.append((time.perf_counter() - t0) * 1e3)
    if gpu:
        after_ingest.append(first_batch(c, pn))
    c.close()
med = statistics.median
print(f"{nn} nodes / {len(pn)} pods / {len(its)} instance types, median of {reps} (min .. max), {os.cpu_count()} host threads visible")
print(f"  one IT= availability flip, continued              {med(update):8.2f} ms  ({min(update):.2f} .. {max(update):.2f})")
print(f"  the snapshot ingested again (parse + flatten)     {med(ingest):8.2f} ms  ({min(ingest):.2f} .. {max(ingest):.2f})")
if gpu:
    print(f"  first 512 what-ifs after the IT=                  {med(after_update):8.2f} ms  ({min(after_update):.2f} .. {max(after_update):.2f})")
    print(f"  first 512 what-ifs after the re-ingest            {med(after_ingest):8.2f} ms  ({min(after_ingest):.2f} .. {max(after_ingest):.2f})")
a.close()
