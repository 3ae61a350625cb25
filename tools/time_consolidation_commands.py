"""Timing of the routes to consolidation commands over BASELINE config #4's shape (512 candidate sets over the 2 048-node snapshot), one process, one GPU, a warm-up
batch first, then the median (and min / max) of RUNS runs of each:
  (a) consolidation.compute_consolidations as it stands: every what-if's full result decoded on the host, then a second trip for price_filter;
  (b) the cheapest ABI-only route there was before ksh_consolidation_commands: what-ifs derived on the device, ksh_solve_batch_resident, ksh_result_records_dev into a
      device buffer and one copy back, ksh_price_filter over the what-ifs with exactly one new node; the candidates' price sums are made outside the timed region;
  (b-dl) the same for a caller without a device buffer: ksh_solve_batch without text (every result read back), ksh_result_summaries, ksh_price_filter;
  (c) ksh_consolidation_commands, with the library's own split (open | solve | command kernel | read-back | host work around them);
  (c-py) consolidation.compute_consolidations_dev: (c) plus what (a) also pays in Python -- the snapshot to KSP1 text and parsed, the rows to Command objects;
  (d) the same three for firstNNodeConsolidationOption over 100 prefixes, where (a) makes one more price_filter call per probed prefix.
(b) and (c) start from a snapshot already parsed (ksh_parse), as a cgo caller holds it.
    python tools/time_consolidation_commands.py [NODES] [WHATIFS] [RUNS]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from karpenter_core_amd import consolidation as C, scheduler as S, workloads as W      # noqa: E402

nodes_n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
n_whatifs = int(sys.argv[2]) if len(sys.argv) > 2 else 512
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 9
its, prov, nodes, bound = W.cluster_snapshot(nodes_n, 50, 45)
snapshot = C.Snapshot(its, prov, nodes, bound)
sets = [list(s) for s in W.config4_sets(n_whatifs, nodes_n, 45)]
prefix_cands = list(range(101))
words = (len(its) + 63) // 64
problem, pod_node = W.snapshot_problem(its, prov, nodes, bound)
parsed = S.ParsedProblem(problem)
types = {it.name: it for it in its}


def stats(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "runs": len(xs)}


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def route_a(css):
    cmds, flats, _ = C.compute_consolidations(snapshot, css)
    for f in flats:
        f.close()
    return [c.action for c in cmds]


def prices_of(css):
    """getNodePrices per candidate set, outside every timed region: (c) sums in C++ inside the call, (b) is handed the sums, so that (b) is not charged for Python."""
    def one(cs):
        try:
            return C.get_node_prices(types, [C.candidate(snapshot, j) for j in cs])
        except ValueError:      # a candidate without an offering: never priced (the reference returns the error first)
            return float("nan")
    return [one(cs) for cs in css]


def route_b(css, prices, second=False):
    """The cheapest ABI-only route before this change: derived open, RESIDENT solve, the fixed-size records built on the device (ksh_result_records_dev) and copied
    back, ksh_price_filter over the what-ifs with exactly one new node."""
    import torch
    flats = S.open_whatifs(parsed, pod_node, css, derive=True)
    try:
        S.solve_batch_resident(flats)
        dev = torch.empty((len(css), 3 + words), dtype=torch.int64, device="cuda:0")
        S.result_records_dev(flats, list(range(len(css))), words, dev)
        rec = dev.cpu().numpy()
        need = [i for i in range(len(css)) if rec[i, 1] == 1 and rec[i, 2] == 0]
        kept = S.price_filter([flats[i] for i in need], [0] * len(need), [prices[i] for i in need])
        if second:      # filterOutSameType's second pricing, batched (the cheapest way to have it before the command kernel)
            S.price_filter([flats[i] for i in need], [0] * len(need), [prices[i] for i in need], [False] * len(need))
        return len(kept)
    finally:
        for f in flats:
            f.close()


def route_b_download(css, prices):
    """(b) as a caller without a device buffer of its own had it: ksh_solve_batch without text (every result read back), ksh_result_summaries, ksh_price_filter."""
    flats = S.open_whatifs(parsed, pod_node, css, derive=True)
    try:
        S.solve_batch(flats, decode=False)
        rec = S.result_records(flats, list(range(len(css))), words)
        need = [i for i in range(len(css)) if rec[i, 1] == 1 and rec[i, 2] == 0]
        return len(S.price_filter([flats[i] for i in need], [0] * len(need), [prices[i] for i in need]))
    finally:
        for f in flats:
            f.close()


def route_c(css):
    rows, ms = S.consolidation_commands(parsed, pod_node, css, words)
    return ms


out = {"nodes": len(nodes), "bound_pods": len(problem.pods), "instance_types": len(its), "whatifs": len(sets), "prefixes": len(prefix_cands) - 1}
set_prices, prefix_prices = prices_of(sets), None
route_a(sets[:64]); route_b(sets, set_prices); route_b_download(sets, set_prices); route_c(sets)                       # warm-up: libraries loaded, the snapshot flattened and resident, the pools filled
a, b, bdl, c, cpy, split = [], [], [], [], [], {k: [] for k in S.COMMAND_TIMING_KEYS}
for _ in range(runs):
    a.append(timed(lambda: route_a(sets))[0])
    b.append(timed(lambda: route_b(sets, set_prices))[0])
    bdl.append(timed(lambda: route_b_download(sets, set_prices))[0])
    t, ms = timed(lambda: route_c(sets))
    c.append(t)
    for k in split:
        split[k].append(ms[k])
    cpy.append(timed(lambda: C.compute_consolidations_dev(snapshot, sets))[0])
out["a_compute_consolidations"] = stats(a)
out["b_abi_before_resident_records_dev"] = stats(b)
out["b_dl_abi_before_full_download"] = stats(bdl)
out["c_ksh_consolidation_commands"] = stats(c)
out["c_split"] = {k: stats(v) for k, v in split.items()}
out["c_py_compute_consolidations_dev"] = stats(cpy)
actions_a = route_a(sets)
actions_c = [cmd.action for cmd in C.compute_consolidations_dev(snapshot, sets)]
out["same_actions"] = actions_a == actions_c
out["actions"] = {x: actions_c.count(x) for x in sorted(set(actions_c))}

prefixes = [prefix_cands[: m + 1] for m in range(1, len(prefix_cands))]
prefix_prices = prices_of(prefixes)
C.first_n_node_consolidation_option(snapshot, prefix_cands, 100); route_b(prefixes, prefix_prices, True); S.first_n_node_option(parsed, pod_node, prefix_cands, words)
da, db, dc, dsplit = [], [], [], {k: [] for k in S.COMMAND_TIMING_KEYS}
for _ in range(runs):
    da.append(timed(lambda: C.first_n_node_consolidation_option(snapshot, prefix_cands, 100))[0])
    db.append(timed(lambda: route_b(prefixes, prefix_prices, True))[0])
    t, (row, ms) = timed(lambda: S.first_n_node_option(parsed, pod_node, prefix_cands, words))
    dc.append(t)
    for k in dsplit:
        dsplit[k].append(ms[k])
out["d_first_n"] = {"a_first_n_node_consolidation_option": stats(da), "b_abi_before_resident_records_dev": stats(db), "c_ksh_first_n_node_option": stats(dc),
                    "c_split": {k: stats(v) for k, v in dsplit.items()}}
row, _ = S.first_n_node_option(parsed, pod_node, prefix_cands, words)
out["d_command"] = {"action": int(row[S.KS_CMD_DECISION]) & 0xFF, "nodes_removed": int(row[S.KS_CMD_ID])}
out["d_same_command"] = C.first_n_node_consolidation_option(snapshot, prefix_cands, 100).canonical() == C.first_n_node_consolidation_option_dev(snapshot, prefix_cands, 100).canonical()
print(json.dumps(out))
