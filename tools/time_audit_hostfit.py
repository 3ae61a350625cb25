#!/usr/bin/env python3
"""The audit's sixth pass (ksolve.h ks_audit_hostfit_dev / ks_audit_hostfit_batch_dev) beside the fourth pass and the Solve it audits: kernel and read-back time on the
same resident result in the same run on the same box, what the pass examined, its count tests, how many (class, node) pairs admitted, its cost per evaluated pair
against the fourth pass's, and whether it found anything.  Needs a GPU.
   usage: tools/time_audit_hostfit.py [legs, comma separated] [reps]      (defaults: config3,whatifs,config5 9)
   legs   config3   BASELINE configs[2]: 100 000 pods / 2 000 types (workloads.config3 seed 44) -- bench.py's contract workload
          whatifs   config #4b's shape with topology: 512 what-ifs derived on the device over the 2 048-node snapshot whose bound pods carry spread / affinity /
                    anti-affinity terms (tests/test_whatif_derived.py's generator, as tools/time_audit_firstfit.py), audited as ONE batch where their results lie
          config5   BASELINE configs[4]'s generator at 250 000 pods / 5 000 types
Per leg: the Solve (its pack kernel time as the library reports it), one untimed call of each pass, then each pass `reps` times: median with min and max of the
kernels' lap (inputs up, the launches, completion) and of the read-back lap, milliseconds."""
import os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from karpenter_core_amd import scheduler as S, workloads as W

legs = (sys.argv[1] if len(sys.argv) > 1 else "config3,whatifs,config5").split(",")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
if S.device_count() < 1:
    sys.exit("time_audit_hostfit.py needs a gfx950 device: there is no CPU path to time")


def stat(xs):
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def report(pack_ms, host, fit):
    """host, fit: [reps] lists of per-problem dicts of one batch, the sixth pass's and the fourth's (the timings are the batch's, in every member)"""
    last, last4 = host[-1], fit[-1]
    flagged = {k: sum(a["pod_bit_count"][k] for a in last) for k in S.KS_AUDIT_HOSTFIT_BITS}
    flagged4 = {k: sum(a["pod_bit_count"][k] for a in last4) for k in S.KS_AUDIT_FIRSTFIT_BITS}
    total, total4 = (lambda k: sum(a["checked"][k] for a in last)), (lambda k: sum(a["checked"][k] for a in last4))
    hk, fk = statistics.median(l[0]["ms"][0] for l in host), statistics.median(l[0]["ms"][0] for l in fit)
    print(f"   hostfit pass kernels     {stat([l[0]['ms'][0] for l in host])}")
    print(f"   hostfit pass read-back   {stat([l[0]['ms'][1] for l in host])}")
    print(f"   first-fit pass kernels   {stat([l[0]['ms'][0] for l in fit])}")
    print(f"   first-fit pass read-back {stat([l[0]['ms'][1] for l in fit])}")
    print(f"   hostfit: checked [{total('SEQ')}, {total('PODS')}, {total('PAIRS')}, {total('TESTS')}] (placed pods, pods examined, (class, node) pairs, count tests); "
          f"admitting_pairs {sum(a['admitting_pairs'] for a in last)}; skipped_pods {sum(a['skipped_pods'] for a in last)}; eligible groups {sum(a['eligible_groups'] for a in last)}, "
          f"skipped {sum(a['skipped_groups'] for a in last)}")
    print(f"   first-fit: checked [{total4('SEQ')}, {total4('PODS')}, {total4('PAIRS')}]; admitting_pairs {sum(a['admitting_pairs'] for a in last4)}")
    per, per4 = (hk * 1e6 / total("PAIRS") if total("PAIRS") else float("nan")), (fk * 1e6 / total4("PAIRS") if total4("PAIRS") else float("nan"))
    print(f"   per evaluated pair: hostfit {per:.3f} ns, first-fit {per4:.3f} ns, ratio {per / per4:.2f};  hostfit / pack kernel {hk / pack_ms * 100:.2f} %, first-fit / pack kernel {fk / pack_ms * 100:.2f} %")
    print(f"   result: hostfit pass {'clean (0 pods flagged)' if not any(flagged.values()) else 'FLAGGED %s' % flagged}; first-fit pass {'clean' if not any(flagged4.values()) else 'FLAGGED %s' % flagged4}", flush=True)


def single(name, problem):
    t0 = time.perf_counter()
    f = S.FlatProblem(problem)
    f.upload(0)
    t1 = time.perf_counter()
    f.solve(decode=False)
    pack_ms, wall_ms = f.kernel_ms, f.wall_ms
    f.solve(decode=False)      # (the second Solve of a resident problem: tables built, kernels loaded)
    pack_ms = min(pack_ms, f.kernel_ms)
    host = [[f.audit_hostfit()] for _ in range(reps + 1)][1:]
    fit = [[f.audit_firstfit()] for _ in range(reps + 1)][1:]
    d = f.dims
    print(f"{name}: {d['P']} pods, {d['T']} types, {d['E']} existing nodes, {d['C']} classes, {d['G']} groups ({d['GH']} on the hostname); {host[0][0]['n_new']} new nodes, "
          f"{host[0][0]['n_placed']} pods placed; ks_pack_rr {f.rr_status()}", flush=True)
    print(f"   flatten + upload {(t1 - t0) * 1e3:.0f} ms; pack kernel {pack_ms:.2f} ms (Solve wall {wall_ms:.2f} ms)")
    report(pack_ms, host, fit)
    f.close()


for leg in legs:
    print(f"--- {leg} (generating) ---", flush=True)
    if leg == "config3":
        single("BASELINE configs[2]", W.config3(pods=100_000, sizes=50, seed=44))
    elif leg == "config5":
        single("BASELINE configs[4] at 250 000 pods", W.config5(pods=250_000, sizes=50, seed=46))
    elif leg == "whatifs":
        from test_whatif_derived import _topology_snapshot      # (the generator of the differential tests)
        its, prov, nodes, bound, snap, pod_node = _topology_snapshot(2048, 50, 45, spare=-1, extras=True, anti=True)
        parsed, sets = S.ParsedProblem(snap), W.config4_sets(512, 2048, 45)
        flats = S.open_whatifs(parsed, pod_node, sets, derive=True)
        S.solve_batch_resident(flats)
        pack_ms, _ = S.solve_batch_resident(flats)
        host = [S.audit_hostfit_batch(flats) for _ in range(reps + 1)][1:]
        fit = [S.audit_firstfit_batch(flats) for _ in range(reps + 1)][1:]
        pods = sum(len(a["pod_flags"]) for a in host[0])
        print(f"config #4b with topology: {len(flats)} what-ifs derived on the device over {len(nodes)} nodes / {len(its)} types; {pods} pods, {sum(a['n_new'] for a in host[0])} new nodes in all", flush=True)
        print(f"   pack kernel (one batched launch) {pack_ms:.2f} ms")
        report(pack_ms, host, fit)
        for f in flats:
            f.close()
    else:
        sys.exit(f"unknown leg {leg}")
