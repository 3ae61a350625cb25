"""Timing of consolidation what-ifs over a cluster with CSI volume limits and claims (`workloads.volume_snapshot`): the route that derives them on the device
with their volumes (KSH_DERIVE_VOLUMES: ks_whatifs_open_ex, per-what-if volume state) against the route that flattens them one by one on the host -- and, for
scale, derived what-ifs over the same cluster without its volumes (`cluster_snapshot`).  Config #4's shape by default.
    python tools/time_whatif_volumes.py [NODES] [WHATIFS]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from karpenter_core_amd import scheduler as S, workloads as W      # noqa: E402

nodes_n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
n_whatifs = int(sys.argv[2]) if len(sys.argv) > 2 else 512
its, prov, nodes, bound = W.volume_snapshot(nodes_n, 50, 45)
snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
plain, plain_pn = W.snapshot_problem(*W.cluster_snapshot(nodes_n, 50, 45), False)
sets = W.config4_sets(n_whatifs, nodes_n, 45)
parsed, parsed_plain = S.ParsedProblem(snap), S.ParsedProblem(plain)
claims = {(v.driver, v.pvc_id) for b in bound for p in b for v in p.volumes}
out = {"nodes": len(nodes), "bound_pods": len(snap.pods), "claims": len(claims), "whatifs": len(sets)}


def run(p, pn, derive, volumes):
    t0 = time.perf_counter()
    flats = S.open_whatifs(p, pn, sets, derive=derive, volumes=volumes)
    t1 = time.perf_counter()
    res, kms, _ = S.solve_batch(flats, decode=False)
    t2 = time.perf_counter()
    words = (len(its) + 63) // 64
    rec = S.result_records(flats, list(range(len(sets))), words)
    t3 = time.perf_counter()
    dims = flats[0].dims
    for f in flats:
        f.close()
    return {"open_ms": (t1 - t0) * 1e3, "solve_ms": (t2 - t1) * 1e3, "kernel_ms": kms, "records_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3}, rec, dims


def arena_bytes(p, pn, volumes):
    """Bytes of the derived batch's device arena (kshost.h ksh_whatifs_arena_bytes): every what-if's mutable state, the volume counts / sets included."""
    flats = S.open_whatifs(p, pn, sets, derive=True, volumes=volumes)
    kh = S.libs()[1]
    kh.ksh_whatifs_arena_bytes.restype = ctypes.c_uint64
    kh.ksh_whatifs_arena_bytes.argtypes = [ctypes.c_void_p]
    b = int(kh.ksh_whatifs_arena_bytes(flats[0]._h))
    for f in flats:
        f.close()
    return b


cold, rd, _ = run(parsed, pod_node, True, True)
warm = [run(parsed, pod_node, True, True)[0] for _ in range(3)]
out["derived_volumes_first_batch"] = cold
out["derived_volumes_warm"] = sorted(warm, key=lambda x: x["total_ms"])[1]
fl, rf, _ = run(parsed, pod_node, False, False)
out["flattened_one_by_one_first"] = fl
out["flattened_one_by_one_warm"] = run(parsed, pod_node, False, False)[0]
out["same_records"] = bool((rd == rf).all())
run(parsed_plain, plain_pn, True, False)
out["derived_without_volumes_warm"] = sorted([run(parsed_plain, plain_pn, True, False)[0] for _ in range(3)], key=lambda x: x["total_ms"])[1]
out["arena_bytes_volumes"] = arena_bytes(parsed, pod_node, True)
out["arena_bytes_without_volumes"] = arena_bytes(parsed_plain, plain_pn, False)
print(json.dumps(out))
