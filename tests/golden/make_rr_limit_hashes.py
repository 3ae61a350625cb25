#!/usr/bin/env python3
"""Golden fingerprints of the node-count cases of tests/rr_limit_cases.py (GOLDEN: thousands of one-pod machines), produced by the CPU oracle alone -- it needs
about three minutes for each, which is why tests/test_rr_limits.py and tests/test_rr_limits_gpu.py compare fingerprints instead of running it.
    python tests/golden/make_rr_limit_hashes.py        # rewrites tests/golden/rr_limit_hashes.json"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import oracle_py as O  # noqa: E402
import rr_limit_cases as RC  # noqa: E402

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rr_limit_hashes.json")
out = json.load(open(path)) if os.path.exists(path) and "--all" not in sys.argv else {}      # (cases already there are kept: pass --all to redo them)
for name in RC.GOLDEN:
    if name in out:
        continue
    p = RC.CASES[name][0]()
    t = time.time()
    r = O.solve(p)
    f = RC.fingerprints(r)
    out[name] = dict(sha256=f["fp"], reasons_sha256=f["reasons"], pods=len(p.pods), new_nodes=len(r.new_nodes), unscheduled=len(r.unscheduled),
                     one_pod_each=RC.one_pod_each(r, len(p.pods)), oracle_seconds=round(time.time() - t, 1))
    print(name, out[name], flush=True)
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
