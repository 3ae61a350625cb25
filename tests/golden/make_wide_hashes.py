"""Golden of tests/test_wide_resources.py: the oracle's result for a mid-size wide problem (workloads.wide_catalogue, 20 000 pods, 500 instance types,
10 resource names).  The fingerprint is sha256 over the canonical result JSON.

    python tests/golden/make_wide_hashes.py            # rewrites tests/golden/wide_hashes.json
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from karpenter_core_amd import workloads as W  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

ARGS = dict(names=10, pods=20_000, types=500, existing=64, seed=2024)


def main():
    res = O.solve(W.wide_catalogue(**ARGS))
    out = {"mid": {"args": ARGS, "sha256": hashlib.sha256(json.dumps(res.canonical(), sort_keys=True).encode()).hexdigest(),
                   "new_nodes": len(res.new_nodes), "unscheduled": len(res.unscheduled)}}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wide_hashes.json")
    json.dump(out, open(path, "w"), indent=1, sort_keys=True)
    print(out)


if __name__ == "__main__":
    main()
