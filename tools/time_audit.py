#!/usr/bin/env python3
"""The audit (ksolve.h ks_audit_dev / ks_audit_batch_dev) beside the Solve it audits: its kernel and read-back time next to the pack kernel time of the same Solve on
the same box, and whether it found anything.  Needs a GPU.
   usage: tools/time_audit.py [legs, comma separated] [reps]      (defaults: config3,whatifs,config5 9)
   legs   config3       BASELINE configs[2]: 100 000 pods / 2 000 types (workloads.config3 seed 44) -- bench.py's contract workload
          whatifs       BASELINE configs[3]: 512 what-ifs derived on the device over the 2 048-node snapshot, audited as ONE batch where their results lie
          config5       BASELINE configs[4]'s generator at 250 000 pods / 5 000 types
          config5_full  the same at the stated 1 000 000 pods (minutes of generation; not part of the default)
Per leg: the Solve once (its pack kernel time as the library reports it), then the audit `reps` times over the same resident result: median with min and max of the
kernels' lap (inputs up, four launches, completion) and of the read-back lap (the flag words to the host and the totals), milliseconds."""
import os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from karpenter_core_amd import scheduler as S, workloads as W

legs = (sys.argv[1] if len(sys.argv) > 1 else "config3,whatifs,config5").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
if S.device_count() < 1:
    sys.exit("time_audit.py needs a gfx950 device: there is no CPU path to time")


def stat(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def findings(audits):
    pods, nodes = sum(a["n_pods_flagged"] for a in audits), sum(a["n_nodes_flagged"] for a in audits)
    if not pods and not nodes:
        return "clean"
    bits = {}
    for a in audits:
        for k, v in list(a["pod_bit_count"].items()) + list(a["node_bit_count"].items()):
            if v:
                bits[k] = bits.get(k, 0) + v
    return f"FLAGGED: {pods} pods, {nodes} nodes {bits}"


def single(name, problem):
    t0 = time.perf_counter()
    f = S.FlatProblem(problem)
    f.upload(0)
    t1 = time.perf_counter()
    f.solve(decode=False)
    pack_ms, wall_ms = f.kernel_ms, f.wall_ms
    f.solve(decode=False)      # (the second Solve of a resident problem: tables built, kernels loaded)
    pack_ms = min(pack_ms, f.kernel_ms)
    laps = [f.audit() for _ in range(reps + 1)][1:]
    d = f.dims
    print(f"{name}: {d['P']} pods, {d['T']} types, {d['E']} existing nodes; {laps[0]['n_new']} new nodes, {laps[0]['n_unscheduled']} unscheduled; ks_pack_rr {f.rr_status()}", flush=True)
    print(f"   flatten + upload {(t1 - t0) * 1e3:.0f} ms; pack kernel {pack_ms:.2f} ms (Solve wall {wall_ms:.2f} ms)")
    print(f"   audit kernels  {stat([a['ms'][0] for a in laps])}")
    print(f"   audit read-back {stat([a['ms'][1] for a in laps])}")
    print(f"   audit / pack kernel: {statistics.median(a['ms'][0] for a in laps) / pack_ms * 100:.2f} %;  result: {findings(laps[-1:])}", flush=True)
    f.close()


for leg in legs:
    print(f"--- {leg} (generating) ---", flush=True)
    if leg == "config3":
        single("BASELINE configs[2]", W.config3(pods=100_000, sizes=50, seed=44))
    elif leg == "config5":
        single("BASELINE configs[4] at 250 000 pods", W.config5(pods=250_000, sizes=50, seed=46))
    elif leg == "config5_full":
        single("BASELINE configs[4] at the stated 1 000 000 pods", W.config5(pods=1_000_000, sizes=50, seed=46))
    elif leg == "whatifs":
        its, prov, nodes, bound = W.cluster_snapshot(2048, 50, 45)
        snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
        parsed, sets = S.ParsedProblem(snap), W.config4_sets(512, 2048, 45)
        flats = S.open_whatifs(parsed, pod_node, sets, derive=True)
        S.solve_batch_resident(flats)
        pack_ms, _ = S.solve_batch_resident(flats)
        laps = [S.audit_batch(flats) for _ in range(reps + 1)][1:]
        pods = sum(len(a["pod_flags"]) for a in laps[0])
        print(f"BASELINE configs[3]: {len(flats)} what-ifs derived on the device over {len(nodes)} nodes / {len(its)} types; {pods} pods, {sum(a['n_new'] for a in laps[0])} new nodes in all", flush=True)
        print(f"   pack kernel (one batched launch) {pack_ms:.2f} ms")
        print(f"   audit kernels  {stat([l[0]['ms'][0] for l in laps])}")
        print(f"   audit read-back {stat([l[0]['ms'][1] for l in laps])}")
        print(f"   audit / pack kernel: {statistics.median(l[0]['ms'][0] for l in laps) / pack_ms * 100:.2f} %;  result: {findings(laps[-1])}", flush=True)
        for f in flats:
            f.close()
    else:
        sys.exit(f"unknown leg {leg}")
