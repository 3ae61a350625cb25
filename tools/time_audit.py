#!/usr/bin/env python3
"""Passes of the audit (ksolve.h ks_audit*_dev / ks_audit*_batch_dev) beside the Solve they audit: kernel and read-back time of each on the same resident result in the
same run on the same box next to the pack kernel time of that Solve, what each pass examined -- `checked` by name and every counter it returns --, and whether it found
anything.  Needs a GPU.
   usage: tools/time_audit.py <pass>[,<pass>] [legs, comma separated] [reps]      (defaults: config3,whatifs,config5 9)
   pass   gate | gate_ex (below) | audit | topology | spread | firstfit | limits | hostfit (scheduler._AUDIT_PASSES) | stages (scheduler._AUDIT_PASSES_BESIDE) | reasons
          (scheduler._AUDIT_PASSES_REASONS) | zonefit (scheduler._AUDIT_PASSES_ZONEFIT; zonefit,hostfit,spread: the ninth pass beside the sixth, its yardstick, and the
          third, whose chunk table it builds again); the first one named is the subject, the others are timed beside it (hostfit,firstfit: the sixth pass beside the fourth,
          with the cost per evaluated pair of each; stages,firstfit: the seventh beside the fourth, whose pair kernels it runs over fewer classes; reasons,audit: the
          eighth beside the first, the other pass that reads no commit numbers)
          gate   the audit's gate (ksh_audit_gate) over the passes named beside it -- all six if it is named alone --, with no findings table: one call, totals
                 reduced on the device.  Timed in the same run as those passes' own calls, and set against their sum.  The what-ifs are `limits`' snapshot
          gate_ex  the wide gate (ksh_audit_gate_ex) over all eight passes, with no findings table, against the cheapest sequence there was before it: the old gate
                 over the six, then the seventh pass's own call, then the eighth's.  The four calls are timed INTERLEAVED -- one round of all four per repetition --
                 and the sequence's time is summed per round.  The what-ifs are `limits`' snapshot
   legs   config3       BASELINE configs[2]: 100 000 pods / 2 000 types (workloads.config3 seed 44) -- bench.py's contract workload; no limited template
          whatifs       512 what-ifs derived on the device over a 2 048-node snapshot, audited as ONE batch where their results lie.  For `audit` BASELINE configs[3]'s
                        snapshot; for the later passes config #4b's shape with topology, the bound pods carrying spread / affinity / anti-affinity terms
                        (tests/test_whatif_derived.py's generator); for `limits` that snapshot's provisioner limited to the cpu its nodes hold
          config5       BASELINE configs[4]'s generator at 250 000 pods / 5 000 types: its `high` provisioner carries a cpu limit
          config5low    the same with that limit divided by eight (for the case that the limit as generated never excludes a type)
          config5_full  config5 at the stated 1 000 000 pods (minutes of generation; not part of the default)
          relax         tests/audit_stages_cases.py's family -- pods whose preferences cannot hold, over three existing nodes -- scaled until some thousand pods relax
          relaxwide     2 000 pods of 2 000 different requests that all relax once, over 1 024 existing nodes: as many distinct earlier-stage classes as pods, so that
                        the pair kernels, not the launches, are what is timed
          zonal         tests/audit_zonefit_cases.py's family -- existing nodes over three zones, pods under zonal spread, some of which open machines -- seed 1 at
                        scale 200: some 2 800 existing nodes and 9 000 pods
          stay          tests/audit_reasons_cases.py's family -- pods that stay unscheduled, each kind on purpose, nine provisioners of mixed kinds over two existing
                        nodes -- scaled until some thousand pods of many hundred classes stay unscheduled
Per leg: the Solve (its pack kernel time as the library reports it), one untimed call of each pass, then each pass `reps` times: median with min and max of the
kernels' lap (inputs up, the launches, completion) and of the read-back lap (the flag words to the host and the totals), milliseconds."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from karpenter_core_amd import fake, scheduler as S, workloads as W

PASSES = dict(S._AUDIT_PASSES, **S._AUDIT_PASSES_BESIDE, **S._AUDIT_PASSES_REASONS, **S._AUDIT_PASSES_ZONEFIT)      # every pass with a call of its own; the gate runs the first table's
if len(sys.argv) < 2 or not all(p in PASSES or p in ("gate", "gate_ex") for p in sys.argv[1].split(",")):
    sys.exit(__doc__)
passes = sys.argv[1].split(",")
gated = [p for p in passes if p in S._AUDIT_PASSES] or list(S._AUDIT_PASSES)      # what the gate runs
if passes == ["gate"]:
    passes += gated
BESIDE = [w for w in S.AUDIT_GATE_ALL if w not in S._AUDIT_PASSES]      # the passes the old gate leaves to calls of their own
if "gate_ex" in passes:
    passes = ["gate_ex", "gate"] + BESIDE
legs = (sys.argv[2] if len(sys.argv) > 2 else "config3,whatifs,config5").split(",")
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
if S.device_count() < 1:
    sys.exit("time_audit.py needs a gfx950 device: there is no CPU path to time")
SIZES = ("n_new", "n_placed", "n_unscheduled")      # (of the result, not of what a pass examined: in the leg's first line)


def stat(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def timed(call):
    """[reps] results of `call` -- each a list of per-problem dicts of one batch, the timings the batch's in every member -- after one untimed"""
    return [call() for _ in range(reps + 1)][1:]


def timed_runs(flats):
    """{pass: timed()} over `flats`: pass after pass -- or, with gate_ex, interleaved: after one untimed call of each, `reps` rounds of one call of each"""
    if "gate_ex" not in passes:
        return {what: timed(lambda: audit(what, flats)) for what in passes}
    for what in passes:
        audit(what, flats)
    runs = {what: [] for what in passes}
    for _ in range(reps):
        for what in passes:
            runs[what].append(audit(what, flats))
    return runs


def audit(what, flats):
    """one timed call: a pass's own, or the gate's -- [its dict], the times in it as in a pass's"""
    if what == "gate_ex":
        return [S.audit_gate(flats, list(S.AUDIT_GATE_ALL), cap_findings=0)]
    return S._audit(what, flats) if what != "gate" else [S.audit_gate(flats, gated, cap_findings=0)]


def report_gate_ex(pack_ms, runs):
    """the wide gate against the three calls, round by round"""
    laps, three = runs["gate_ex"], ["gate"] + BESIDE
    wall = [sum(l[0]["ms"]) for l in laps]
    seq_k = [sum(runs[w][i][0]["ms"][0] for w in three) for i in range(len(laps))]
    seq_r = [sum(runs[w][i][0]["ms"][1] for w in three) for i in range(len(laps))]
    seq = [k + r for k, r in zip(seq_k, seq_r)]
    print(f"   gate_ex ({', '.join(S.AUDIT_GATE_ALL)}) kernels   {stat([l[0]['ms'][0] for l in laps])}")
    print(f"   gate_ex read-back {stat([l[0]['ms'][1] for l in laps])}")
    print(f"   gate_ex kernels + read-back {stat(wall)}; / pack kernel {statistics.median(wall) / pack_ms * 100:.2f} %")
    print(f"   the three calls (gate over the six, {', '.join(BESIDE)}), summed per round: kernels {stat(seq_k)}")
    print(f"   the three calls read-back {stat(seq_r)}")
    print(f"   the three calls kernels + read-back {stat(seq)}")
    print(f"   gate_ex / the three calls: kernels + read-back {statistics.median(wall) / statistics.median(seq):.3f}, kernels {statistics.median(l[0]['ms'][0] for l in laps) / statistics.median(seq_k):.3f}, "
          f"read-back {statistics.median(l[0]['ms'][1] for l in laps) / statistics.median(seq_r):.3f}; gate_ex max {max(wall):.3f} ms against the three calls' min {min(seq):.3f} ms")
    last = laps[-1][0]
    print(f"   result: gate_ex {'clean' if last['clean'] else 'FOUND %d' % last['n_findings']}", flush=True)


def report_gate(pack_ms, runs):
    laps = runs["gate"]
    wall = [sum(l[0]["ms"]) for l in laps]
    print(f"   gate ({', '.join(gated)}) kernels   {stat([l[0]['ms'][0] for l in laps])}")
    print(f"   gate read-back {stat([l[0]['ms'][1] for l in laps])}")
    print(f"   gate kernels + read-back {stat(wall)}; / pack kernel {statistics.median(wall) / pack_ms * 100:.2f} %")
    own = [w for w in gated if w in runs]
    if own == gated:
        k, r = (sum(statistics.median(l[0]["ms"][i] for l in runs[w]) for w in own) for i in (0, 1))
        print(f"   the {len(own)} calls' own, summed medians: kernels {k:.3f} ms, read-back {r:.3f} ms, kernels + read-back {k + r:.3f} ms")
        print(f"   gate / the calls: kernels + read-back {statistics.median(wall) / (k + r):.3f}, read-back {statistics.median(l[0]['ms'][1] for l in laps) / r:.3f}")
    last = laps[-1][0]
    print(f"   result: gate {'clean' if last['clean'] else 'FOUND %d' % last['n_findings']}", flush=True)


def report(pack_ms, runs):
    """runs: {pass: timed()}"""
    per_pair = {}
    if "gate_ex" in runs:
        report_gate_ex(pack_ms, runs)
    if "gate" in runs:
        report_gate(pack_ms, runs)
    for what, laps in runs.items():
        if what in ("gate", "gate_ex"):
            continue
        p, last = PASSES[what], laps[-1]
        kernels, both = statistics.median(l[0]["ms"][0] for l in laps), statistics.median(sum(l[0]["ms"]) for l in laps)
        print(f"   {what} kernels   {stat([l[0]['ms'][0] for l in laps])}")
        print(f"   {what} read-back {stat([l[0]['ms'][1] for l in laps])}")
        print(f"   {what} / pack kernel: kernels {kernels / pack_ms * 100:.2f} %, kernels + read-back {both / pack_ms * 100:.2f} %")
        checked = {k: sum(a["checked"][k] for a in last) for k in p["checked"] or ()}
        counters = {k: sum(a[k] for a in last) for k in p["scalars"] if k not in SIZES}
        if checked or counters:
            print(f"   {what}: checked {checked}; " + "; ".join(f"{k} {v}" for k, v in counters.items()))
        if checked.get("PAIRS") or checked.get("ZONE"):      # (the ninth pass counts its (pod, node) pairs under ZONE: the zone test runs on every one)
            per_pair[what] = kernels * 1e6 / (checked.get("PAIRS") or checked["ZONE"])
        flagged = {k: sum(a[t][k] for a in last) for t, bits in (("pod_bit_count", p["pod_bits"]), ("node_bit_count", p["node_bits"] or {})) for k in bits}
        print(f"   result: {what} {'clean (nothing flagged)' if not any(flagged.values()) else 'FLAGGED %s' % {k: v for k, v in flagged.items() if v}}", flush=True)
    if len(per_pair) > 1:      # (passes that count (class, node) pairs, side by side)
        first = next(iter(per_pair.values()))
        print("   per evaluated pair: " + ", ".join(f"{w} {ns:.3f} ns" for w, ns in per_pair.items()) + "".join(f"; {next(iter(per_pair))} / {w} {first / ns:.2f}" for w, ns in list(per_pair.items())[1:]), flush=True)


def single(name, problem):
    t0 = time.perf_counter()
    f = S.FlatProblem(problem)
    f.upload(0)
    t1 = time.perf_counter()
    f.solve(decode=False)
    pack_ms, wall_ms = f.kernel_ms, f.wall_ms
    f.solve(decode=False)      # (the second Solve of a resident problem: tables built, kernels loaded)
    pack_ms = min(pack_ms, f.kernel_ms)
    runs = timed_runs([f])
    d, first = f.dims, runs[[p for p in passes if p not in ("gate", "gate_ex")][0]][0][0]
    print(f"{name}: {d['P']} pods, {d['T']} types, {d['E']} existing nodes, {d['C']} classes, {d['M']} templates, {d['G']} topology groups ({d['GH']} on the hostname); "
          + ", ".join(f"{k} {first[k]}" for k in SIZES if k in first) + f"; ks_pack_rr {f.rr_status()}", flush=True)
    print(f"   flatten + upload {(t1 - t0) * 1e3:.0f} ms; pack kernel {pack_ms:.2f} ms (Solve wall {wall_ms:.2f} ms)")
    report(pack_ms, runs)
    f.close()


def whatifs():
    if passes[0] == "audit":
        its, prov, nodes, bound = W.cluster_snapshot(2048, 50, 45)
        snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
        name = "BASELINE configs[3]"
    else:
        from test_whatif_derived import _topology_snapshot      # (the generator of the differential tests)
        its, prov, nodes, bound, snap, pod_node = _topology_snapshot(2048, 50, 45, spare=-1, extras=True, anti=True)
        name = "config #4b with topology"
        if passes[0] in ("limits", "gate", "gate_ex"):
            limit = {"cpu": str(int(sum(fake._qty_value(n.capacity.get("cpu", "0")) for n in nodes)))}
            for p in snap.provisioners:
                p.limits = dict(limit)
            name += f", provisioner limited to {limit}"
    flats = S.open_whatifs(S.ParsedProblem(snap), pod_node, W.config4_sets(512, 2048, 45), derive=True)
    S.solve_batch_resident(flats)
    pack_ms, _ = S.solve_batch_resident(flats)
    runs = timed_runs(flats)
    first = runs[[p for p in passes if p not in ("gate", "gate_ex")][0]][0]
    print(f"{name}: {len(flats)} what-ifs derived on the device over {len(nodes)} nodes / {len(its)} types; {sum(len(a['pod_flags']) for a in first)} pods, "
          f"{sum(a['n_new'] for a in first)} new nodes in all", flush=True)
    print(f"   pack kernel (one batched launch) {pack_ms:.2f} ms")
    report(pack_ms, runs)
    for f in flats:
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
    elif leg == "config5_full":
        single("BASELINE configs[4] at the stated 1 000 000 pods", W.config5(pods=1_000_000, sizes=50, seed=46))
    elif leg == "whatifs":
        whatifs()
    elif leg == "relax":
        import audit_stages_cases
        single("the relaxing family, seed 3 with existing nodes, scale 400", audit_stages_cases.relax_problem(3, True, scale=400))
    elif leg == "relaxwide":
        import audit_stages_cases
        single("2 000 relaxing pods of 2 000 classes over 1 024 existing nodes", audit_stages_cases.many_relaxed(2000, nodes=1024))
    elif leg == "zonal":
        import audit_zonefit_cases
        single("the zonal family, seed 1 at scale 200", audit_zonefit_cases.zonal_cluster(1, scale=200))
    elif leg == "stay":
        import audit_reasons_cases
        single("the unscheduled family, seed 7 with nine provisioners and existing nodes, scale 300", audit_reasons_cases.stay_problem(**dict(audit_reasons_cases.FAMILY[6][1], scale=300)))
    else:
        sys.exit(f"unknown leg {leg}")
