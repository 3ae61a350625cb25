#!/usr/bin/env python3
"""what the snapshot's flattening costs after a one-node change, continued (ksh_env_apply) against from scratch -- host only, no GPU needed.
   usage: tools/time_env_apply.py [nodes] [reps] [--binary]      env KSH_TIMING=1 prints the phases
   --binary: the same event lists through both doors, into two snapshots -- the KSD1 text (ksh_env_apply) and the delta block (ksh_env_apply_block): the library's
   decode + apply time of each (the apply is shared and dominates; the decode is what differs), and what the caller spends building the text / the block in Python."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
from karpenter_core_amd import model as M, scheduler as S, workloads as W
args = [a for a in sys.argv[1:] if not a.startswith("--")]
binary = "--binary" in sys.argv[1:]
nn = int(args[0]) if len(args) > 0 else 2048
reps = int(args[1]) if len(args) > 1 else 5
its, prov, nodes, bound = W.cluster_snapshot(nn, 50, 45)
snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
parsed = S.ParsedProblem(snap)
t = time.perf_counter(); parsed.snapshot_fingerprint(pn); cold0 = (time.perf_counter() - t) * 1e3
from test_env_apply import new_node
rs = np.random.RandomState(3)
if binary:
    twin = S.ParsedProblem(snap); twin.snapshot_fingerprint(pn)
warm, cold, blk, build_text, build_block = [], [], [], [], []
for r in range(reps):
    name = f"late-{r}"
    ev = [("node+", new_node(its, name, rs))] + [("bind", name, W.generic_pod(rs, f"late-{r}-{k}")) for k in range(20)]
    if os.environ.get("KSH_TIMING"): sys.stderr.write(f"--- apply {r}\n")
    if binary:      # (the door that goes second runs while the first one's previous flattening is torn down on another thread: the order alternates)
        t = time.perf_counter(); M.delta_to_ksd(ev).encode(); build_text.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); block = M.delta_to_block(ev); build_block.append((time.perf_counter() - t) * 1e3)
    for door in (["text", "block"] if r % 2 == 0 else ["block", "text"]) if binary else ["text"]:
        if os.environ.get("KSH_TIMING"): sys.stderr.write(f"--- {door} door, apply {r}\n")
        if door == "text":
            info = parsed.apply(ev, pn if r == 0 else None)
            assert info["continued"], info
            warm.append(info["ms"])
        else:
            ib = twin.apply_block(block, pn if r == 0 else None)
            assert ib["continued"], ib
            blk.append(ib["ms"])
    if binary:
        assert twin.snapshot_fingerprint() == parsed.snapshot_fingerprint()
    t = time.perf_counter(); parsed.snapshot_fingerprint(cold=True); cold.append((time.perf_counter() - t) * 1e3)
print(f"snapshot: {nn} nodes, {len(pn)} bound pods | first flattening {cold0:.1f} ms | after one node + 20 pods: continued {statistics.median(warm):.2f} ms (min {min(warm):.2f}), "
      f"from scratch + hash {statistics.median(cold):.1f} ms")
if binary:
    print(f"both doors, the same {reps} event lists (1 NODE+ and 20 BIND each; which door goes first alternates), decode + apply in the library: text door (ksh_env_apply) {statistics.median(warm):.2f} ms (min {min(warm):.2f}) | "
          f"binary door (ksh_env_apply_block) {statistics.median(blk):.2f} ms (min {min(blk):.2f}) | same flattening after every call | "
          f"building the events in Python: KSD1 text {statistics.median(build_text):.2f} ms, delta block {statistics.median(build_block):.2f} ms")
