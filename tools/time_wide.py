#!/usr/bin/env python3
"""Kernel time of a wide problem (workloads.wide_catalogue, R > 8: the wide ks_pack variant) and of its stripped twin (the same pods and catalogue without
the names nothing requests, R <= 8: today's kernels), on the GPU.  Each Solve is warmed once, then timed `--reps` times by the library's device events
(FlatProblem.kernel_ms: the static tables + the pack kernel); the line per problem gives the median and the spread.

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


def timed(pr, reps):
    f = S.FlatProblem(pr)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    print(f"# kernel ms per Solve (median of {a.reps}, min-max), wide problem vs its stripped twin on the same pods")
    for kw in CASES:
        wide, ww, wr, wms = timed(W.wide_catalogue(**kw), a.reps)
        twin, tw, tr, tms = timed(W.wide_catalogue(strip=True, **kw), a.reps)
        same = len(wide.new_nodes) == len(twin.new_nodes) and wide.unscheduled == twin.unscheduled
        print(f"{str(kw):80s} wide R={wr:2d} ks_pack RM={ww:2d} {statistics.median(wms):9.3f} ms ({min(wms):.3f}-{max(wms):.3f})   "
              f"twin R={tr} RM={tw} {statistics.median(tms):9.3f} ms ({min(tms):.3f}-{max(tms):.3f})   ratio {statistics.median(wms) / statistics.median(tms):.3f}"
              f"   nodes {len(wide.new_nodes)} unscheduled {len(wide.unscheduled)} same={same}", flush=True)


if __name__ == "__main__":
    main()
