"""Timing of command validation over BASELINE config #4's shape: 512 commands over the 2 048-node snapshot, after a one-node change (NODE-) applied as an event.  One
process, one GPU, a warm-up of each route first, then RUNS runs of the two routes INTERLEAVED; median and min / max of each:
  (new) ksh_validate_commands, with the library's own split (open | solve | validation kernel | read-back | host work around them);
  (old) the cheapest sequence the ABI offered before it for the same answers: ksh_open_whatifs_derived over the mapped node sets, ksh_solve_batch_resident,
        ksh_result_records_dev into a device buffer and one copy back, ksh_types_subset over the commands that expect a replacement and got exactly one node.  The
        mapping (which nodes of a command are still candidates) and the readiness rule are computed OUTSIDE the timed region for this route.
The commands are the rows ksh_consolidation_commands gave a pass earlier for tools/time_consolidation_commands.py's candidate sets: a replace expects its options, every
other row is validated as a delete of its set.  Candidates (`why`) come from ksh_consolidation_candidates over the changed snapshot, outside both timed regions.
    python tools/bench_validation.py [NODES] [COMMANDS] [RUNS]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from karpenter_core_amd import scheduler as S, workloads as W      # noqa: E402

nodes_n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
n_cmds = int(sys.argv[2]) if len(sys.argv) > 2 else 512
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 9
its, prov, nodes, bound = W.cluster_snapshot(nodes_n, 50, 45)
sets = [list(s) for s in W.config4_sets(n_cmds, nodes_n, 45)]
words = (len(its) + 63) // 64
problem, pod_node = W.snapshot_problem(its, prov, nodes, bound)
parsed = S.ParsedProblem(problem)


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


# t0: the commands
rows, _ = S.consolidation_commands(parsed, pod_node, sets, words)
expect = [(int(r[S.KS_CMD_DECISION]) & 0xFF) == S.KS_CMD_REPLACE for r in rows]
type_sets = [[w * 64 + b for w in range(words) for b in range(64) if (int(r[S.KS_CMD_OPTIONS + w]) >> b) & 1] if e else [] for r, e in zip(rows, expect)]
# the change: the node most commands do not name leaves
named = {c for cs in sets for c in cs}
gone = max(i for i in range(len(nodes)) if i not in named)
parsed.apply([("node-", nodes[gone].name)], pod_node)
bind, n_slots = parsed.bindings()
nf = [0] * n_slots
cand = S.consolidation_candidates(parsed, None, nf, [0.0] * n_slots, [0] * len(bind), [0.0] * len(bind), [0] * len(bind), [True], [None])
why = [int(x) for x in cand["why"]]
mapped = [sorted({c for c in cs if why[c] in (0, 10, 11, 12)}) for cs in sets]
live = [i for i, m in enumerate(mapped) if m]
unready = [i for i, n in enumerate(nodes) if i != gone and n.labels.get("karpenter.sh/initialized") != "true" and n.labels.get("karpenter.sh/provisioner-name")]


def route_new():
    return S.validate_commands(parsed, None, sets, expect, type_sets, why, nf, words)


def route_old():
    import torch
    flats = S.open_whatifs(parsed, None, [mapped[i] for i in live], derive=True)
    try:
        S.solve_batch_resident(flats)
        dev = torch.empty((len(live), 3 + words), dtype=torch.int64, device="cuda:0")
        S.result_records_dev(flats, live, words, dev)
        rec = dev.cpu().numpy()
        need = [k for k, i in enumerate(live) if rec[k, 1] == 1 and rec[k, 2] == 0 and expect[i]]
        sub = S.types_subset([flats[k] for k in need], [0] * len(need), [type_sets[live[k]] for k in need])
        return rec, need, sub
    finally:
        for f in flats:
            f.close()


def verdicts_old(rec, need, sub):
    out = [False] * len(sets)
    ok = dict(zip(need, sub))
    for k, i in enumerate(live):
        blocked = any(u not in mapped[i] for u in unready)
        if blocked or rec[k, 2]:
            continue
        out[i] = (not expect[i]) if rec[k, 1] == 0 else (rec[k, 1] == 1 and expect[i] and ok.get(k, False))
    return out


route_new(); route_old()          # warm-up: the changed snapshot flattened and resident, the pools filled
new, old, split = [], [], {k: [] for k in S.COMMAND_TIMING_KEYS}
for _ in range(runs):
    t, (vrows, ms) = timed(route_new)
    new.append(t)
    for k in split:
        split[k].append(ms[k])
    t, got_old = timed(route_old)
    old.append(t)
valid_new = [(int(r[S.KS_VAL_VERDICT]) & 0xFF) == S.KS_VAL_VALID for r in vrows]
whys = [(int(r[S.KS_VAL_VERDICT]) >> 8) & 0xFF for r in vrows]
out = {"nodes": len(nodes), "bound_pods": len(problem.pods), "instance_types": len(its), "commands": len(sets), "expect_replacement": sum(expect), "node_removed": nodes[gone].name,
       "new_ksh_validate_commands": stats(new), "new_split": {k: stats(v) for k, v in split.items()}, "old_open_solve_records_subset": stats(old),
       "ratio_new_over_old": statistics.median(new) / statistics.median(old), "same_verdicts": valid_new == verdicts_old(*got_old),
       "why": {str(w): whys.count(w) for w in sorted(set(whys))}}
print(json.dumps(out))
parsed.close()
