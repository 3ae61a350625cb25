"""Timing of the FIRST step of an expiration pass over the 2 048-node snapshot of tools/bench_validation.py, all nodes expired: which nodes are candidates and in what order.

  new     ksh_deprovisioning_candidates(KSH_METHOD_EXPIRATION): the filter in int64 nanoseconds and the sort by expiration time on the device.
  parent  the cheapest route for the same order before that call existed: ksh_consolidation_candidates for the node filter (codes 0, 10-12), then the expiration filter
          and the stable sort in Python over the arrays it returns.

Then the WHOLE pass -- new: that call + ksh_replacement_option (one what-if simulated); parent: the route above + consolidation.replacement_command, which simulates every
candidate in one GPU batch and decodes on the host -- and the 512-set ksh_replacement_commands batch against ksh_consolidation_commands over the same sets (the same solves;
the difference is the two replacement kernels and the read-back of the node table).  All six run interleaved in one process, median of `runs` with min and max, after one
warm-up of each; the two routes' answers are compared before anything is timed.  Prints one JSON line."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from karpenter_core_amd import scheduler as S, workloads as W      # noqa: E402

nodes_n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 9
its, prov, nodes, bound = W.cluster_snapshot(nodes_n, 50, 45)
problem, pod_node = W.snapshot_problem(its, prov, nodes, bound)
parsed = S.ParsedProblem(problem)
n_pods = len(pod_node)
SECOND, NOW, TTL = 10 ** 9, 1_700_000_000 * 10 ** 9, 3600
created = [NOW - (TTL + 1 + (i * 7919) % 1000) * SECOND for i in range(nodes_n)]      # every node expired, 1 000 distinct expiration times: keys repeat
age = [(NOW - c) / SECOND for c in created]
nf, pf, dc, pp = [0] * nodes_n, [0] * n_pods, [0.0] * n_pods, [0] * n_pods


def route_new():
    return S.deprovisioning_candidates(parsed, S.KSH_METHOD_EXPIRATION, pod_node, NOW, nf, created, age, pf, dc, pp, [TTL])["order"]


def route_parent():
    got = S.consolidation_candidates(parsed, pod_node, nf, age, pf, dc, pp, [True], [TTL])
    why = got["why"]
    live = [i for i in range(nodes_n) if why[i] == 0 and NOW > created[i] + TTL * SECOND]
    return sorted(live, key=lambda i: created[i] + TTL * SECOND)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


# ---- the whole pass: candidates + ComputeCommand.  New: ONE what-if simulated.  Parent: consolidation.replacement_command simulates every candidate it is given in one GPU batch
from karpenter_core_amd import consolidation as C      # noqa: E402
words = (len(its) + 63) // 64
snapshot = C.Snapshot(its, prov, nodes, bound)


def pass_new():
    got = S.deprovisioning_candidates(parsed, S.KSH_METHOD_EXPIRATION, pod_node, NOW, nf, created, age, pf, dc, pp, [TTL])
    head, rows, total, pos, _ = S.replacement_option(parsed, pod_node, got["order"], got["why"], words)
    return got["order"][pos], int(head[S.KS_REP_DECISION]) & 0xFF, total


def pass_parent():
    action, removed, replacements = C.replacement_command(snapshot, route_parent())
    return removed, action, len(replacements)


# ---- the 512-set batch: the same solves, then the two replacement kernels + both tables read back, against the command kernel + its rows read back
sets = [list(x) for x in W.config4_sets(512, nodes_n, 45)]


def batch_new():
    return S.replacement_commands(parsed, pod_node, sets, words, cap_nodes=8 * len(sets))[2]


def batch_commands():
    return S.consolidation_commands(parsed, pod_node, sets, words)[0]


a, b = route_new(), route_parent()      # warm-up, and the check that both routes answer the same question
assert a == b and len(a) > 0, (len(a), len(b))
pn, pp_ = pass_new(), pass_parent()
assert nodes[pn[0]].name == pp_[0][0], (pn, pp_)      # the same node decides on both routes
tot = batch_new(); batch_commands()
assert tot <= 8 * len(sets), tot
t_new, t_parent, t_pnew, t_pparent, t_bnew, t_bcmd = [], [], [], [], [], []
for _ in range(runs):
    t_new.append(timed(route_new)[0])
    t_parent.append(timed(route_parent)[0])
    t_pnew.append(timed(pass_new)[0])
    t_pparent.append(timed(pass_parent)[0])
    t_bnew.append(timed(batch_new)[0])
    t_bcmd.append(timed(batch_commands)[0])
print(json.dumps({"nodes": nodes_n, "pods": n_pods, "candidates": len(a), "new_candidates": stats(t_new), "parent_candidates": stats(t_parent),
                  "pass_new_candidates_plus_replacement_option": stats(t_pnew), "pass_parent_candidates_plus_replacement_command": stats(t_pparent), "decided": {"node": nodes[pn[0]].name, "action": pn[1], "new_nodes": pn[2]},
                  "batch_512_replacement_commands": stats(t_bnew), "batch_512_consolidation_commands": stats(t_bcmd), "batch_512_total_node_rows": tot}))
parsed.close()
