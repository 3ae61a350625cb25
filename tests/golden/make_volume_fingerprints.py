#!/usr/bin/env python3
"""Fingerprints of the flag-0 flattenings of three `workloads.volume_snapshot` clusters, made before what-ifs over volume snapshots could be derived on the
device (KSH_DERIVE_VOLUMES): the snapshot's own flattening (ksh_snapshot_fingerprint, flags 0) and four what-ifs flattened on the host over it (ksh_fingerprint).
tests/test_whatif_volumes.py::test_flag0_flattening_of_volume_snapshots_is_unchanged holds the library to them: the opt-in route builds a flattening of its own
and must leave these bytes alone.  Regenerate only after a DELIBERATE change of the flag-0 encoding:  python tests/golden/make_volume_fingerprints.py"""
import json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE))); sys.path.insert(0, os.path.dirname(HERE))

CASES = {"vol-48x5-s1": (48, 5, 1), "vol-96x6-s2": (96, 6, 2), "vol-160x8-s3": (160, 8, 3)}
SETS = [[0], [1, 2, 3], [5, 0], list(range(12))]


def compute():
    from karpenter_core_amd import scheduler as S, workloads as W
    out = {}
    for name, (existing, sizes, seed) in CASES.items():
        snap, pod_node = W.snapshot_problem(*W.volume_snapshot(existing, sizes, seed), True)
        parsed = S.ParsedProblem(snap)
        out[name + "/snapshot"] = "%016x" % parsed.snapshot_fingerprint(pod_node)
        for i, f in enumerate(S.open_whatifs(parsed, pod_node, SETS, derive=False)):
            out[f"{name}/whatif-{i}"] = "%016x" % f.fingerprint()
            f.close()
        parsed.close()
    return out


if __name__ == "__main__":
    json.dump(compute(), open(os.path.join(HERE, "volume_fingerprints.json"), "w"), indent=0, sort_keys=True)
    print("written")
