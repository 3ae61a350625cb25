#!/usr/bin/env python3
"""The audit's fifth pass (ksolve.h ks_audit_limits_dev / ks_audit_limits_batch_dev) beside the Solve it audits: kernel and read-back time on the same resident
result on the same box, what the pass examined, how many nodes were exact, on how many the limit excluded a type, and whether it found anything.  Needs a GPU.
   usage: tools/time_audit_limits.py [legs, comma separated] [reps]      (defaults: config3,whatifs,config5 9)
   legs   config3     BASELINE configs[2]: 100 000 pods / 2 000 types (workloads.config3 seed 44) -- no limited template: the pass's early-out
          whatifs     config #4b's shape with topology: 512 what-ifs derived on the device over the 2 048-node snapshot whose bound pods carry spread / affinity /
                      anti-affinity terms (tests/test_whatif_derived.py's generator, as tools/time_audit_firstfit.py), the snapshot's provisioner limited to the cpu
                      its nodes hold, audited as ONE batch where their results lie
          config5     BASELINE configs[4]'s generator at 250 000 pods / 5 000 types: its `high` provisioner carries a cpu limit
          config5low  the same with that limit divided by eight (for the case that the limit as generated never excludes a type)
Per leg: the Solve (its pack kernel time as the library reports it), one untimed call of the pass, then the pass `reps` times: median with min and max of the
kernels' lap (inputs up, the launches, completion) and of the read-back lap, milliseconds."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from karpenter_core_amd import fake, scheduler as S, workloads as W

legs = (sys.argv[1] if len(sys.argv) > 1 else "config3,whatifs,config5").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
if S.device_count() < 1:
    sys.exit("time_audit_limits.py needs a gfx950 device: there is no CPU path to time")


def stat(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def report(pack_ms, runs):
    """runs: [reps] lists of per-problem dicts of one batch (the timings are the batch's, in every member)"""
    last = runs[-1]
    flagged = {k: sum(a["pod_bit_count"][k] for a in last) for k in S.KS_AUDIT_LIMITS_POD_BITS}
    flagged.update({k: sum(a["node_bit_count"][k] for a in last) for k in S.KS_AUDIT_LIMITS_NODE_BITS})
    total = lambda k: sum(a["checked"][k] for a in last)
    tot = lambda k: sum(a[k] for a in last)
    print(f"   limits pass kernels   {stat([l[0]['ms'][0] for l in runs])}")
    print(f"   limits pass read-back {stat([l[0]['ms'][1] for l in runs])}")
    both = statistics.median(l[0]['ms'][0] + l[0]['ms'][1] for l in runs)
    print(f"   limits pass (kernels + read-back) / pack kernel: {both / pack_ms * 100:.2f} %;  limited_templates {tot('limited_templates')}; checked [{total('SEQ')}, {total('NODES')}, "
          f"{total('PODS')}, {total('PAIRS')}] (placed pods, nodes of limited templates, pods examined, (class, template) pairs)")
    print(f"   exact_nodes {tot('exact_nodes')}; binding_nodes {tot('binding_nodes')}; skipped_nodes {tot('skipped_nodes')}; skipped_pods {tot('skipped_pods')}")
    print(f"   result: limits pass {'clean (nothing flagged)' if not any(flagged.values()) else 'FLAGGED %s' % flagged}", flush=True)


def single(name, problem):
    t0 = time.perf_counter()
    f = S.FlatProblem(problem)
    f.upload(0)
    t1 = time.perf_counter()
    f.solve(decode=False)
    pack_ms, wall_ms = f.kernel_ms, f.wall_ms
    f.solve(decode=False)      # (the second Solve of a resident problem: tables built, kernels loaded)
    pack_ms = min(pack_ms, f.kernel_ms)
    runs = [[f.audit_limits()] for _ in range(reps + 1)][1:]
    d = f.dims
    print(f"{name}: {d['P']} pods, {d['T']} types, {d['E']} existing nodes, {d['C']} classes, {d['M']} templates; {runs[0][0]['n_new']} new nodes, {runs[0][0]['n_placed']} pods placed; "
          f"ks_pack_rr {f.rr_status()}", flush=True)
    print(f"   flatten + upload {(t1 - t0) * 1e3:.0f} ms; pack kernel {pack_ms:.2f} ms (Solve wall {wall_ms:.2f} ms)")
    report(pack_ms, runs)
    f.close()


for leg in legs:
    print(f"--- {leg} (generating) ---", flush=True)
    if leg == "config3":
        single("BASELINE configs[2]", W.config3(pods=100_000, sizes=50, seed=44))
    elif leg in ("config5", "config5low"):
        pr = W.config5(pods=250_000, sizes=50, seed=46)
        for p in pr.provisioners:
            if p.limits and leg == "config5low":
                p.limits = {k: str(int(fake._qty_value(v)) // 8) for k, v in p.limits.items()}
        print("   limits: " + ", ".join(f"{p.name} {p.limits}" for p in pr.provisioners))
        single("BASELINE configs[4] at 250 000 pods" + (", the limit divided by eight" if leg == "config5low" else ""), pr)
    elif leg == "whatifs":
        from test_whatif_derived import _topology_snapshot      # (the generator of the differential tests)
        its, prov, nodes, bound, snap, pod_node = _topology_snapshot(2048, 50, 45, spare=-1, extras=True, anti=True)
        limit = {"cpu": str(int(sum(fake._qty_value(n.capacity.get("cpu", "0")) for n in nodes)))}
        for p in snap.provisioners:
            p.limits = dict(limit)
        parsed, sets = S.ParsedProblem(snap), W.config4_sets(512, 2048, 45)
        flats = S.open_whatifs(parsed, pod_node, sets, derive=True)
        S.solve_batch_resident(flats)
        pack_ms, _ = S.solve_batch_resident(flats)
        runs = [S.audit_limits_batch(flats) for _ in range(reps + 1)][1:]
        pods = sum(len(a["pod_flags"]) for a in runs[0])
        print(f"config #4b with topology, provisioner limited to {limit}: {len(flats)} what-ifs derived on the device over {len(nodes)} nodes / {len(its)} types; {pods} pods, "
              f"{sum(a['n_new'] for a in runs[0])} new nodes in all", flush=True)
        print(f"   pack kernel (one batched launch) {pack_ms:.2f} ms")
        report(pack_ms, runs)
        for f in flats:
            f.close()
    else:
        sys.exit(f"unknown leg {leg}")
