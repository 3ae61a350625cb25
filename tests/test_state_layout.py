"""The host half of csrc/ksolve.hip lays a Solve's mutable state out ONCE (`state_layout`, for an uploaded problem and for the what-ifs derived from a snapshot) and
names the result arrays ONCE (`KS_RESULT_SEGS`, for the single-Solve and the batched read-back).  What that must keep:

  - the device arena of a derived batch is, byte for byte, as large as before the layouts were merged (literals below);
  - nothing a kernel reads of the uninitialised region depends on what was there: every what-if of five tiny batches -- no topology, zonal + hostname groups,
    volumes, a batch of one, host ports -- and an uploaded problem with two hostname groups equal the oracle under KS_POISON = 0x00, 0xFF, 0xA5;
  - a problem solved alone (`download`: one transfer per array) and as the first member of a batch (`ks_gather`: one blob) reads back the same bytes.

The kernels run in a child process: on the emulator build (tests/sim) for the CPU legs, on the device under `-m gpu`."""
import ctypes
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import workloads as W
from karpenter_core_amd.model import (DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_ZONE, Container, HostPort, LabelSelector, TopologySpreadConstraint)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POISONS = ["0x00", "0xFF", "0xA5"]


# ---------------------------------------------------------------------------------------------------------------- the batches: 6 nodes, at most 36 bound pods
def _cluster(seed, spare, existing=6, per_node=6):
    """`cluster_snapshot` cut down: `existing` nodes with at most `per_node` bound pods each; `spare` nodes keep free pod slots, the others are full by pod count."""
    its, prov, nodes, bound = W.cluster_snapshot(existing, 4, seed, spare_pod_slots=spare)
    return its, prov, nodes, [b[:per_node] for b in bound]


def _spread(p, label, key, skew):
    p.labels = {"my-label": label}
    p.spread = [TopologySpreadConstraint(skew, key, DO_NOT_SCHEDULE, LabelSelector({"my-label": label}))]


def build_batch(name):
    """(snapshot problem, pod_node, per-node bound pods, candidate sets, derive with volumes)"""
    if name == "plain":
        its, prov, nodes, bound = _cluster(11, 2)
        sets = [[0], [1, 2], [5, 3, 4]]
    elif name == "topology":      # one zonal and one hostname-keyed spread group, owned by pods on every node
        its, prov, nodes, bound = _cluster(12, 2)
        for pods in bound:
            if len(pods) > 0:
                _spread(pods[0], "a", LABEL_ZONE, 1)
            if len(pods) > 1:
                _spread(pods[1], "b", LABEL_HOSTNAME, 2)
        sets = [[0], [1, 2], [5, 3, 4]]
    elif name == "volumes":
        its, prov, nodes, bound = _cluster(13, 2)
        W.decorate_volumes(nodes, bound, np.random.RandomState(13))
        sets = [[0], [2, 4]]
    elif name == "one":
        its, prov, nodes, bound = _cluster(14, 0)
        sets = [[0, 1, 2]]
    elif name == "ports":         # a node holds a port once (hostportusage.go:122-144): a pod that leaves its node must not land where its port is taken
        its, prov, nodes, bound = _cluster(15, 2)
        rs = np.random.RandomState(15)
        for n, pods in zip(nodes, bound):
            taken = []
            for p in pods:
                port = 9000 + int(rs.randint(3))
                if rs.rand() < 0.5 and port not in taken:
                    p.containers[0].ports = [HostPort(port=port)]
                    taken.append(port)
            n.host_ports = [hp for p in pods for hp in p.containers[0].ports]
        sets = [[0], [1, 2], [5, 3, 4]]
    else:
        raise KeyError(name)
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, name == "topology")
    assert len(snap.nodes) == 6 and len(snap.pods) <= 40
    return snap, pod_node, bound, sets, name == "volumes"


BATCHES = ["plain", "topology", "volumes", "one", "ports"]


def whatif_problem(snap, bound, cs):
    """simulateScheduling's problem for one candidate set: the what-if flattened by itself."""
    cand = set(cs)
    return dataclasses.replace(snap, pods=[p for i in cs for p in bound[i]], nodes=[dataclasses.replace(n, in_state=i not in cand) for i, n in enumerate(snap.nodes)])


def uploaded_problem():
    """Not derived: a problem uploaded from the host, whose pods own two hostname-keyed spread groups (`hcnt` comes 0xFF-filled there)."""
    its, prov, nodes, bound = _cluster(16, 1)
    for pods in bound:
        for i, p in enumerate(pods):
            _spread(p, "ab"[i % 2], LABEL_HOSTNAME, 1 + i % 2)
    return W.whatif(its, prov, nodes, bound, [0, 1], True)


# ---------------------------------------------------------------------------------------------------------------- the read-back pairs: at most 30 pods, 4 existing nodes
def readback_pair(shape):
    """(A, B): A is solved alone and as the first member of [A, B]."""
    partner = W.config2(pods=14, sizes=1, seed=2)      # (another K, several templates, 7 new nodes)
    if shape == "odd":            # N = 3 new nodes, K = 3 keys: N * K * 4 bytes end off an 8-byte boundary
        return W.hostname_herd(pods=9, labels=3, seed=3), partner
    if shape == "n0":             # every pod lands on an existing node
        its, prov, nodes, bound = _cluster(11, -1, existing=4)
        return W.whatif(its, prov, nodes, bound, [0], False), partner
    if shape == "r9":             # nine resource names: the wide row
        return W.wide_catalogue(names=9, pods=20, types=24, existing=4, seed=1), partner
    if shape == "unschedulable":
        pr = W.config3(pods=12, sizes=4, seed=7)
        big = dataclasses.replace(pr.pods[0], uid="too-big", containers=[Container(requests={"cpu": "100000", "memory": "1Gi"})])
        return dataclasses.replace(pr, pods=pr.pods + [big]), partner
    if shape == "mixed":          # P 14 and 25, TW 3 and 1: the members' offsets in the blob differ
        its, prov, nodes, bound = _cluster(12, 0, existing=4, per_node=7)
        return W.whatif(its, prov, nodes, bound, [0, 1, 2, 3], False), W.config1(pods=25, types=40, seed=3)
    raise KeyError(shape)


SHAPES = ["odd", "n0", "r9", "unschedulable", "mixed"]


class _RA(ctypes.Structure):      # include/kshost.h ksh_result_arrays
    _fields_ = [(n, ctypes.c_uint32) for n in ("n_pods", "n_existing", "n_new", "n_unscheduled", "types_words", "n_resources", "n_keys", "pad")] + \
               [(n, ctypes.c_void_p) for n in ("pod_node", "pod_stage", "pod_reason", "unscheduled", "node_pods_off", "node_pods", "node_tmpl", "node_types", "node_requests",
                                               "node_requests_present", "node_present", "node_complement", "node_mask", "node_gt", "node_lt", "node_it_state")]


def all_result_arrays(Sm, fp):
    """`FlatProblem.result_arrays()` and the three arrays of the binary door it leaves out (node_gt, node_lt, node_it_state): every result array, as hex of its bytes.
    (pod_seq comes through node_pods, which is ordered by it.)"""
    ra = fp.result_arrays()
    out = {k: np.ascontiguousarray(v).tobytes().hex() for k, v in ra.items() if isinstance(v, np.ndarray)}
    out["n_new"] = int(ra["n_new"])
    raw = _RA()
    assert Sm.libs()[1].ksh_result_arrays_get(fp._h, ctypes.byref(raw)) == 0
    for name, n in (("node_gt", raw.n_new * raw.n_keys), ("node_lt", raw.n_new * raw.n_keys), ("node_it_state", raw.n_new)):
        ptr = getattr(raw, name)
        out[name] = ctypes.string_at(ptr, 4 * n).hex() if n and ptr else ""
    return out


# ---------------------------------------------------------------------------------------------------------------- the part that needs the kernels
def _plain(r):
    return [r.canonical(), sorted(r.reasons.items())]


def device_run(Sm, job):
    if job["kind"] == "derived":
        snap, pod_node, bound, sets, volumes = build_batch(job["name"])
        parsed = Sm.ParsedProblem(snap)
        derived = Sm.open_whatifs(parsed, pod_node, sets, derive=True, volumes=volumes)
        try:
            kh = Sm.libs()[1]
            kh.ksh_whatifs_arena_bytes.restype, kh.ksh_whatifs_arena_bytes.argtypes = ctypes.c_uint64, [ctypes.c_void_p]
            got, _, _ = Sm.solve_batch(derived)
            return {"arena": int(kh.ksh_whatifs_arena_bytes(derived[0]._h)), "dims": derived[0].dims, "results": [_plain(r) for r in got]}
        finally:
            for f in derived:
                f.close()
            parsed.close()
    if job["kind"] == "uploaded":
        fp = Sm.FlatProblem(uploaded_problem())
        try:
            return {"dims": fp.dims, "results": [_plain(fp.solve())]}
        finally:
            fp.close()
    a, b = readback_pair(job["name"])
    fa, fb = Sm.FlatProblem(a), Sm.FlatProblem(b)
    try:
        fa.solve(decode=False)
        alone = all_result_arrays(Sm, fa)
        alone_result = _plain(fa.result())
        Sm.solve_batch([fa, fb], decode=False)
        return {"dims": [fa.dims, fb.dims], "alone": alone, "batched": all_result_arrays(Sm, fa), "alone_result": alone_result, "batched_result": _plain(fa.result())}
    finally:
        fa.close()
        fb.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_state_layout as L
out = {}
for name, job in jobs["jobs"].items():
    try:
        out[name] = L.device_run(S, job)
    except Exception as e:
        out[name] = {"error": repr(e)[:400]}
print("RESULT " + json.dumps(out))
"""


def run_in_child(jobs, sim, tmp, extra_env=None):
    """All `jobs` in ONE fresh process (KS_POISON is read at every upload, but the pytest process keeps its own libraries); a child that dies leaves every job an error."""
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    env.pop("KS_POISON", None)
    env.update(extra_env or {})
    path = os.path.join(tmp, f"jobs_{len(os.listdir(tmp))}.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "jobs": jobs}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=600)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in jobs}
    return json.loads(line[-1][7:])


LAYOUT_JOBS = dict({name: {"kind": "derived", "name": name} for name in BATCHES}, uploaded={"kind": "uploaded"})
READBACK_JOBS = {shape: {"kind": "readback", "name": shape} for shape in SHAPES}
_RUNS = {}


def run(request, backend, jobs, poison=None):
    """One child per (backend, job set, poison byte), shared by the tests of the module."""
    key = (backend, tuple(jobs), poison)
    if key not in _RUNS:
        sim = backend == "emu" or bool(os.environ.get("KS_TEST_SIM"))
        tmp = request.getfixturevalue("tmp_path_factory").mktemp("state_layout")
        _RUNS[key] = run_in_child(jobs, sim, str(tmp), {"KS_POISON": poison} if poison else None)
    return _RUNS[key]


_ORACLE = {}


def oracle(name):
    from oracle import oracle_py as O
    if name not in _ORACLE:
        if name == "uploaded":
            problems = [uploaded_problem()]
        elif name in SHAPES:
            problems = [readback_pair(name)[0]]
        else:
            snap, pod_node, bound, sets, volumes = build_batch(name)
            problems = [whatif_problem(snap, bound, cs) for cs in sets]
        _ORACLE[name] = [json.loads(json.dumps(_plain(O.solve(pr)))) for pr in problems]
    return _ORACLE[name]


# ---------------------------------------------------------------------------------------------------------------- arena sizes
# Recorded by running this very test on the commit before `state_layout` existed (three hand-kept layouts): ksh_whatifs_arena_bytes of the five batches.  Every piece
# of the arena is 256-byte aligned, so the order of the pieces cannot move the sum: a difference means a piece was gained, lost or resized.
ARENA_BYTES = {"plain": 36096, "topology": 46592, "volumes": 25856, "one": 24576, "ports": 34560}


def test_whatif_arena_sizes_are_those_of_the_hand_kept_layouts(request):
    res = run(request, "emu", LAYOUT_JOBS, POISONS[0])
    assert all("error" not in res[name] for name in BATCHES), res
    assert {name: res[name]["arena"] for name in BATCHES} == ARENA_BYTES


# ---------------------------------------------------------------------------------------------------------------- uninitialised memory
@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", BATCHES + ["uploaded"])
def test_results_do_not_depend_on_the_uninitialised_region(request, backend, poison, name):
    """canonical() and reasons of every what-if (of the uploaded problem) == the oracle on the what-if flattened by itself, whatever byte fills the region no upload writes."""
    got = run(request, backend, LAYOUT_JOBS, poison)[name]
    assert "error" not in got, got
    if name == "topology":
        assert got["dims"]["G"] > 0 and got["dims"]["GH"] > 0
    if name == "uploaded":
        assert got["dims"]["GH"] >= 2
    assert got["results"] == oracle(name), (name, poison)


# ---------------------------------------------------------------------------------------------------------------- the two read-back paths
@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("shape", SHAPES)
def test_single_and_batched_readback_agree(request, backend, shape):
    """Problem A alone (one transfer per result array) and as the first member of [A, B] (gathered into one blob on the device): every result array byte for byte, and the oracle."""
    got = run(request, backend, READBACK_JOBS)[shape]
    assert "error" not in got, got
    da, db = got["dims"]
    n_new = got["alone"]["n_new"]
    assert da["P"] <= 30 and db["P"] <= 30 and da["E"] <= 4 and db["E"] <= 4
    if shape == "odd":
        assert n_new % 2 == 1 and da["K"] % 2 == 1 and (n_new * da["K"] * 4) % 8 != 0
    if shape == "n0":
        assert n_new == 0 and da["P"] > 0
    if shape == "r9":
        assert da["R"] == 9
    if shape == "unschedulable":
        assert len(bytes.fromhex(got["alone"]["unscheduled"])) >= 4
    if shape == "mixed":
        assert da["P"] != db["P"] and (da["T"] + 63) // 64 != (db["T"] + 63) // 64
    assert set(got["alone"]) == set(got["batched"]) and len(got["alone"]) == 17      # 16 arrays of the binary door (the 15 read back; pod_seq as node_pods_off / node_pods) + n_new
    for k in got["alone"]:
        assert got["alone"][k] == got["batched"][k], (shape, k)
    assert got["alone_result"] == got["batched_result"] == oracle(shape)[0]
