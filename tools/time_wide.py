#!/usr/bin/env python3
"""Kernel time of a wide problem (workloads.wide_catalogue, R > 8: the wide ks_pack variant) and of its stripped twin (the same pods and catalogue without
the names nothing requests, R <= 8: today's kernels), on the GPU.  Each Solve is warmed once, then timed `--reps` times by the library's device events
(FlatProblem.kernel_ms: the static tables + the pack kernel); the line per problem gives the median and the spread, and the same
wide problem flattened with KSH_ACTIVE_RESOURCES (the library doing the stripping) beside them.  --cloud: BASELINE configs[2] under a 12-name catalogue, Solve from the pod list,
flag off / on / undressed interleaved in one process, and the LEAN-at-8 leg (profiles/r09_active_resources.txt).

    python tools/time_wide.py [--reps 7] > profiles/<tag>_wide.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from karpenter_core_amd import scheduler as S, workloads as W  # noqa: E402

CASES = [dict(names=10, pods=20_000, types=500, existing=64, seed=2024), dict(names=16, pods=20_000, types=500, existing=64, seed=2024),
         dict(names=12, pods=2_000, types=100, existing=16, seed=7)]


def timed(pr, reps, active_resources=False):
    f = S.FlatProblem(pr, active_resources=active_resources)
    try:
        res = f.solve()
        width = f.pack_width()
        ms = []
        for _ in range(reps):
            f.solve(decode=False)
            ms.append(f.kernel_ms)
        return res, width, f.dims["R"], ms
    finally:
        f.close()


def from_pods(legs, reps):
    """`Solve` from the pod list (scheduler.solve_from_pods: flatten + upload + tables + pack kernel + read-back) of several legs over parsed objects, INTERLEAVED in
    this one process: every leg once as warm-up, then `reps` rounds of every leg in turn.  Per leg: R, what ran, medians and min-max of pack_kernel_ms and flatten_ms."""
    parsed = [(name, S.ParsedProblem(pr), kw) for name, pr, kw in legs]
    ms = {name: {"pack_kernel_ms": [], "flatten_ms": [], "total_ms": []} for name, _, _ in legs}
    what = {}
    for rep in range(reps + 1):
        for name, pp, kw in parsed:
            f, t = S.solve_from_pods(pp, **kw)
            started, why = f.rr_status()
            what[name] = (f.dims["R"], "ks_pack_rr" if started and why == 0 else f"ks_pack RM={f.pack_width()}{' LEAN' if f.pack_lean() else ''}")
            f.close()
            if rep:
                for k in ms[name]:
                    ms[name][k].append(t[k])
    for name, pp, _ in parsed:
        pp.close()
        m = ms[name]
        col = lambda k: f"{k} {statistics.median(m[k]):9.3f} ({min(m[k]):.3f}-{max(m[k]):.3f})"
        print(f"{name:44s} R={what[name][0]:2d} {what[name][1]:18s} {col('pack_kernel_ms')}   {col('flatten_ms')}   {col('total_ms')}", flush=True)


def cloud(a):
    """BASELINE configs[2] dressed in a 12-name catalogue (workloads.cloud_catalogue): flag off (R = 12, the wide single-wave variant) against KSH_ACTIVE_RESOURCES
    (R = 3, the undressed problem's flat problem byte for byte) against the UNDRESSED problem, the yardstick.  Then the five-name leg -- the same plus an
    ephemeral-storage daemonset and 1 % GPU pods -- under the flag: the LEAN variant at RM = 8 against KS_FLAG_NO_LEAN (the general variant)."""
    import copy
    from karpenter_core_amd.model import Container, Pod
    pr = W.config3(pods=a.pods, sizes=a.sizes, seed=44)
    dressed = W.cloud_catalogue(pr, 12)
    print(f"# Solve from the pod list, {a.pods} pods / {len(pr.instance_types)} types (workloads.config3 seed 44), ms: median of {a.reps} (min-max), legs interleaved in one process")
    from_pods([("undressed, flag off (yardstick)", pr, {}), ("dressed 12 names, flag off", dressed, {}), ("dressed 12 names, KSH_ACTIVE_RESOURCES", dressed, {"active_resources": True})], a.reps)
    five = copy.deepcopy(pr)
    for it in five.instance_types:
        it.capacity["ephemeral-storage"] = "100Gi"
    for i, p in enumerate(five.pods):
        if i % 100 == 37:
            p.containers[0].limits["nvidia.com/gpu"] = "1"
    for i, it in enumerate(five.instance_types):
        if i % 4 == 3:
            it.capacity["nvidia.com/gpu"] = "4"
    five.daemonset_pods = list(five.daemonset_pods) + [Pod(uid="ds-es", containers=[Container(requests={"cpu": "50m", "memory": "32Mi", "ephemeral-storage": "512Mi"})])]
    five = W.cloud_catalogue(five, 12)
    f, g = S.FlatProblem(five, active_resources=True), S.FlatProblem(five, active_resources=True, flags=S.KS_FLAG_NO_LEAN)
    try:
        x, y = f.solve(), g.solve()
        print(f"# five active names: R={f.dims['R']}, same result under both variants: {x.canonical() == y.canonical()}")
        for name, h in (("five names, flag on: LEAN at RM = 8", f), ("five names, flag on + KS_FLAG_NO_LEAN", g)):
            ms = []
            for _ in range(a.reps):
                h.solve(decode=False)
                ms.append(h.kernel_ms)
            print(f"{name:44s} R={h.dims['R']:2d} ks_pack RM={h.pack_width()}{' LEAN' if h.pack_lean() else '':5s} kernel_ms {statistics.median(ms):9.3f} ({min(ms):.3f}-{max(ms):.3f})", flush=True)
    finally:
        f.close(); g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cloud", action="store_true", help="configs[2] under a 12-name catalogue, KSH_ACTIVE_RESOURCES off / on / undressed, and the LEAN-at-8 leg")
    ap.add_argument("--pods", type=int, default=100_000)
    ap.add_argument("--sizes", type=int, default=50)
    a = ap.parse_args()
    if a.cloud:
        return cloud(a)
    print(f"# kernel ms per Solve (median of {a.reps}, min-max), wide problem vs its stripped twin on the same pods")
    for kw in CASES:
        wide, ww, wr, wms = timed(W.wide_catalogue(**kw), a.reps)
        twin, tw, tr, tms = timed(W.wide_catalogue(strip=True, **kw), a.reps)
        same = len(wide.new_nodes) == len(twin.new_nodes) and wide.unscheduled == twin.unscheduled
        on, ow, orr, oms = timed(W.wide_catalogue(**kw), a.reps, active_resources=True)
        same = same and len(on.new_nodes) == len(wide.new_nodes) and on.unscheduled == wide.unscheduled
        print(f"{str(kw):80s} wide R={wr:2d} ks_pack RM={ww:2d} {statistics.median(wms):9.3f} ms ({min(wms):.3f}-{max(wms):.3f})   "
              f"twin R={tr} RM={tw} {statistics.median(tms):9.3f} ms ({min(tms):.3f}-{max(tms):.3f})   ratio {statistics.median(wms) / statistics.median(tms):.3f}   "
              f"flag on R={orr} RM={ow} {statistics.median(oms):9.3f} ms ({min(oms):.3f}-{max(oms):.3f})"
              f"   nodes {len(wide.new_nodes)} unscheduled {len(wide.unscheduled)} same={same}", flush=True)


if __name__ == "__main__":
    main()
