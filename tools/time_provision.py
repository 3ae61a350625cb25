#!/usr/bin/env python3
"""A provisioning pass over the snapshot kept by events (kshost.h ksh_provision) against the road it replaces (ksh_solve_from_batch over an environment whose cache an
event has just dropped).  Needs a GPU.
   usage: tools/time_provision.py [nodes] [reps] [batch sizes, comma separated] [--full]      (defaults: 2048 9 200,2000,20000)
   --full: the snapshot that is full by pod count (config #4b: cluster_snapshot(spare_pod_slots=3)) -- nearly every pending pod then needs a NEW machine
Shape: config #4's snapshot (cluster_snapshot(nodes, 50, 45): 2 048 nodes / 39 242 bound pods / 2 000 types) plus an empty carrier node; per repetition a one-node
change (NODE+) and a burst of B pending pods.
  new road   ksh_env_apply_block(NODE+, B x BIND to the carrier) + ksh_provision, over a snapshot that is flattened, resident and warm (one pass before the window)
  old road   ksh_pods_ingest(B pods) + ksh_env_apply_block(NODE+) on the environment + ksh_solve_from_batch (its flattening of the environment falls inside the
             window: the event dropped the cache)
Building the blocks in Python is outside both windows.  Pod slots are never reused, so every repetition starts from a snapshot parsed anew (outside the window).  A
burst beyond the snapshot's spare pod room is refused by the BIND; the tool says so and then times ksh_provision over a snapshot INGESTED with the burst bound.
Median of `reps` with min-max, milliseconds; both roads must count the same machines and unscheduled pods."""
import dataclasses, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from karpenter_core_amd import model as M, scheduler as S, workloads as W
from karpenter_core_amd.model import StateNode

args = [a for a in sys.argv[1:] if not a.startswith("--")]
full = "--full" in sys.argv[1:]
nn = int(args[0]) if len(args) > 0 else 2048
reps = int(args[1]) if len(args) > 1 else 9
sizes = [int(x) for x in (args[2] if len(args) > 2 else "200,2000,20000").split(",")]
CARRIER = "~pending~"
if S.device_count() < 1:
    sys.exit("time_provision.py needs a gfx950 device: there is no CPU path to time")
its, prov, nodes, bound = W.cluster_snapshot(nn, 50, 47, spare_pod_slots=3) if full else W.cluster_snapshot(nn, 50, 45)
words = (len(its) + 63) // 64
carrier = len(nodes)


def snapshot_text(pending):
    snap, pn = W.snapshot_problem(its, prov, nodes + [StateNode(name=CARRIER)], bound + [list(pending)], False)
    return snap.to_ksp().encode(), pn


def stat(xs):
    return f"{statistics.median(xs):9.2f} ms (min {min(xs):.2f}, max {max(xs):.2f})"


text0, pn0 = snapshot_text([])
env_text = dataclasses.replace(W.snapshot_problem(its, prov, nodes, bound, False)[0], pods=[]).to_ksp().encode()
print(f"snapshot{' (full by pod count)' if full else ''}: {nn} nodes, {len(pn0)} bound pods, {len(its)} instance types; {reps} repetitions per batch size")
for B in sizes:
    new_ms, apply_ms, prov_ms, old_ms, old_flat, old_kernel, parts = [], [], [], [], [], [], []
    mode = "events"
    for r in range(reps):
        rs = np.random.RandomState(1000 * B + r)
        pending = [W.generic_pod(rs, f"burst-{B}-{r}-{k:05d}") for k in range(B)]
        change = ("node+", W.fresh_node(its, f"late-{B}-{r}", rs))
        block = M.delta_to_block([change] + [("bind", CARRIER, p) for p in pending])
        # ---- new road ----
        parsed = S.ParsedProblem.from_text(text0)
        parsed.apply_block([("bind", CARRIER, W.generic_pod(rs, f"warm-{B}-{r}"))], pn0)
        S.provision(parsed, None, [carrier], words)      # flattened, resident, kernels loaded
        parsed.apply_block([("unbind", f"warm-{B}-{r}")])
        try:
            t0 = time.perf_counter()
            info = parsed.apply_block(block)
            t1 = time.perf_counter()
        except S.KSolveError as e:
            if "spare room" not in str(e):
                raise
            if r == 0:
                print(f"B = {B}: the BIND events are refused -- {str(e)[:160]}")
            mode = "ingested"
            parsed.close()
            text_b, pn_b = snapshot_text(pending)
            parsed = S.ParsedProblem.from_text(text_b)
            parsed.apply_block([("bind", CARRIER, W.generic_pod(rs, f"warm-{B}-{r}"))], pn_b)
            S.provision(parsed, None, [carrier], words, cap_rows=0, cap_machines=0)
            parsed.apply_block([("unbind", f"warm-{B}-{r}")])
            t0 = time.perf_counter()
            info = parsed.apply_block([change])
            t1 = time.perf_counter()
        got = S.provision(parsed, None, [carrier], words, cap_rows=B, cap_machines=B)
        t2 = time.perf_counter()
        assert got["total_rows"] == B and got["rows"] is not None and got["machines"] is not None, got["head"]
        new_ms.append((t2 - t0) * 1e3); apply_ms.append((t1 - t0) * 1e3); prov_ms.append((t2 - t1) * 1e3); parts.append(got["ms"])
        route, continued = got["route"], info["continued"]
        parsed.close()
        # ---- old road ----
        env = S.ParsedProblem.from_text(env_text)
        warm = S.PodBatch(M.pods_to_blocks([W.generic_pod(rs, f"warm2-{B}-{r}")]))
        fp, _ = S.solve_from_batch(env, warm); fp.close(); warm.close()
        blocks, eblock = M.pods_to_blocks(pending), M.delta_to_block([change])
        t0 = time.perf_counter()
        batch = S.PodBatch(blocks)
        env.apply_block(eblock, [])
        fp, ms = S.solve_from_batch(env, batch)
        t1 = time.perf_counter()
        res = fp.result()
        assert (len(res.new_nodes), len(res.unscheduled)) == (got["head"]["n_new"], got["head"]["n_unscheduled"]), ((len(res.new_nodes), len(res.unscheduled)), got["head"])
        old_ms.append((t1 - t0) * 1e3); old_flat.append(ms["flatten_ms"]); old_kernel.append(ms["pack_kernel_ms"])
        rr = fp.rr_status()
        fp.close(); batch.close(); env.close()
    med = lambda k: statistics.median(p[k] for p in parts)
    label = mode if mode == "events" else "INGESTED with the burst bound: no BIND inside the new road's window while the old road still ingests its pods -- not like for like"
    print(f"B = {B:6d} ({label}; {got['head']['n_new']} machines, {got['head']['n_unscheduled']} unscheduled; what-if {route}, flattening continued: {continued})")
    print(f"   new road  apply_block + ksh_provision {stat(new_ms)} = apply {stat(apply_ms)} + provision {stat(prov_ms)}")
    print(f"             ksh_provision's laps (medians): open {med('open_ms'):.2f} | solve {med('solve_ms'):.2f} | table kernels {med('command_kernel_ms'):.2f} | read-back {med('readback_ms'):.2f} | host {med('host_ms'):.2f}")
    print(f"   old road  ingest + apply_block + ksh_solve_from_batch {stat(old_ms)}   (flatten {statistics.median(old_flat):.2f}, pack kernel {statistics.median(old_kernel):.2f}; ks_pack_rr {rr})")
    print(f"   ratio old / new (medians): {statistics.median(old_ms) / statistics.median(new_ms):.2f}" + ("" if mode == "events" else "   (not like for like: see above)"))
