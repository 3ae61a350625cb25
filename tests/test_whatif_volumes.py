"""Consolidation what-ifs over snapshots with CSI volume limits and claims, DERIVED on the device (kshost.h KSH_DERIVE_VOLUMES, ksolve.h ks_whatifs_open_ex):
the snapshot is flattened once with a claim partition that holds for every candidate set (solo claims count, multi claims are bits), and every
what-if carries its own per-node volume counts and sets.  The route is opt-in (`volumes=True`); the flag-0 flattening must not move a byte.

CPU: the derived what-ifs run on the emulator build of the kernels (tests/sim) in a child process -- the pytest process keeps the real libraries -- and must
equal the what-ifs flattened on the host and the oracle; the derivation's host restatement (`check_whatif_derivation(volumes=True)`) holds on hundreds of
(snapshot, candidate set) pairs; events applied to the snapshot leave the flagged flattening equal to one made from scratch.  GPU (`-m gpu`): the same families on
the device, config #4's shape (512 what-ifs over 2 048 nodes) record for record with the price stage, a batch of one (the multi-wave kernel), a poisoned arena."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_ZONE, LabelSelector, TopologySpreadConstraint

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---------------------------------------------------------------------------------------------------------------- snapshots
def wide_volume_snapshot(names, seed, existing=24):
    """The wide catalogue (`names` resource names) as a cluster: the generator's pods bound round robin to its existing nodes, decorated like `volume_snapshot`."""
    pr = W.wide_catalogue(names=names, pods=6 * existing, existing=existing, seed=seed, dense=True)
    if pr.provisioners[1].limits:
        pr.provisioners[1].limits.pop("cpu", None)
    pods = [p for p in pr.pods if p.containers[0].requests.get("cpu") != "200"]
    bound = [pods[i::existing] for i in range(existing)]
    nodes = [dataclasses.replace(n) for n in pr.nodes[:existing]]
    W.decorate_volumes(nodes, bound, np.random.RandomState(seed))
    return pr.instance_types, pr.provisioners, nodes, bound, pr


def build_case(spec):
    """(snapshot problem, pod_node, per-node bound pods) of a case spec: ["plain", existing, sizes, seed] | ["topology", existing, sizes, seed] | ["wide", names, seed]."""
    kind = spec[0]
    if kind == "wide":
        its, provs, nodes, bound, pr = wide_volume_snapshot(spec[1], spec[2])
        pod_node = [i for i in range(len(nodes)) for _ in bound[i]]
        snap = dataclasses.replace(pr, nodes=[dataclasses.replace(n, in_state=True) for n in nodes], pods=[p for b in bound for p in b], cluster_pods=[],
                                   simulation_mode=True)
        return snap, pod_node, bound
    its, prov, nodes, bound = W.volume_snapshot(spec[1], spec[2], spec[3])
    if kind == "topology":      # spread terms on a few workloads, the bound pods listed as cluster pods (countDomains)
        rs = np.random.RandomState(spec[3])
        for pods in bound:
            for p in pods:
                lab = p.labels.get("my-label", "")
                if lab == "a":
                    p.spread = [TopologySpreadConstraint(1, LABEL_ZONE, DO_NOT_SCHEDULE, LabelSelector({"my-label": "a"}))]
                elif lab == "b" and rs.rand() < 0.7:
                    p.spread = [TopologySpreadConstraint(3, LABEL_HOSTNAME, DO_NOT_SCHEDULE, LabelSelector({"my-label": "b"}))]
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, kind == "topology")
    return snap, pod_node, bound


def whatif_problem(snap, bound, cs):
    """simulateScheduling's problem for one candidate set (what `workloads.whatif` builds), from the snapshot problem."""
    cand = set(cs)
    return dataclasses.replace(snap, pods=[p for i in cs for p in bound[i]], nodes=[dataclasses.replace(n, in_state=i not in cand) for i, n in enumerate(snap.nodes)])


def candidate_sets(spec, n_nodes, bound):
    """singletons (one of them the last node: for `volume_snapshot`, the node no provisioner owns), prefixes, every node, and sets without pods."""
    rs = np.random.RandomState(1000 + sum(int(x) for x in spec[1:]))
    empty = [i for i, b in enumerate(bound) if not b][:1]
    return ([[int(rs.randint(n_nodes))], [int(rs.randint(n_nodes))], [n_nodes - 1], list(range(2)), list(range(n_nodes // 3)), list(range(n_nodes)), [],
             empty or [], [int(x) for x in rs.choice(n_nodes, size=min(5, n_nodes), replace=False)]])


# 16 volume snapshots, one over the 14-resource catalogue, one with topology terms
CASES = {f"vol-{s}": ["plain", 24 + 5 * s, 4 + s % 5, 300 + s] for s in range(16)}
CASES["wide-14"] = ["wide", 14, 3]
CASES["topology"] = ["topology", 40, 6, 77]


# ---------------------------------------------------------------------------------------------------------------- the part that needs the kernels
def device_run(Sm, job):
    """Open the case's what-ifs derived with their volumes and flattened on the host, solve both; plain data out."""
    snap, pod_node, bound = build_case(job["spec"])
    sets = job["sets"]
    parsed = Sm.ParsedProblem(snap)
    derived = Sm.open_whatifs(parsed, pod_node, sets, derive=True, volumes=True)
    flat = Sm.open_whatifs(parsed, pod_node, sets, derive=False)
    try:
        got, _, _ = Sm.solve_batch(derived)
        want, _, _ = Sm.solve_batch(flat)
        return {"derived": [[r.canonical(), sorted(r.reasons.items())] for r in got], "flat": [[r.canonical(), sorted(r.reasons.items())] for r in want]}
    finally:
        for f in derived + flat:
            f.close()
        parsed.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_whatif_volumes as V
out = {}
for name, job in jobs["jobs"].items():
    try:
        out[name] = V.device_run(S, job)
    except Exception as e:
        out[name] = {"error": repr(e)[:400]}
print("RESULT " + json.dumps(out))
"""


def run_in_child(jobs, sim, tmp, extra_env=None):
    """All `jobs` in ONE fresh process; a child that dies leaves every one of its jobs an error."""
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    env.update(extra_env or {})
    path = os.path.join(tmp, f"jobs_{len(os.listdir(tmp))}.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "jobs": jobs}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in jobs}
    return json.loads(line[-1][7:])


def all_jobs():
    jobs = {}
    for name, spec in CASES.items():
        snap, pod_node, bound = build_case(spec)
        jobs[name] = {"spec": spec, "sets": candidate_sets(spec, len(snap.nodes), bound)}
    return jobs


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return run_in_child(all_jobs(), True, str(tmp_path_factory.mktemp("whatif_volumes_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return run_in_child(all_jobs(), bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("whatif_volumes_gpu")))


_ORACLE = {}


def oracle_results(name):
    from oracle import oracle_py as O
    if name not in _ORACLE:
        spec = CASES[name]
        snap, pod_node, bound = build_case(spec)
        _ORACLE[name] = [O.solve(whatif_problem(snap, bound, cs)) for cs in candidate_sets(spec, len(snap.nodes), bound)]
    return _ORACLE[name]


def check_case(res, name):
    got = res[name]
    assert "error" not in got, got
    refs = oracle_results(name)
    assert len(got["derived"]) == len(got["flat"]) == len(refs)
    for i, ((dc, dr), (fc, fr), ref) in enumerate(zip(got["derived"], got["flat"], refs)):
        want = json.loads(json.dumps([ref.canonical(), sorted(ref.reasons.items())]))
        assert [dc, dr] == [fc, fr], (name, i, "derived != flattened on the host")
        assert [dc, dr] == want, (name, i, "derived != the oracle")


@pytest.mark.parametrize("backend", ["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
@pytest.mark.parametrize("name", list(CASES))
def test_derived_volume_whatifs_match_flattened_and_oracle(request, backend, name):
    """Placements, relaxation stages, InstanceTypeOptions, requirements and reasons of every what-if: derived with volumes == flattened on the host == oracle."""
    check_case(request.getfixturevalue(backend), name)


# ---------------------------------------------------------------------------------------------------------------- CPU: the derivation restated
@pytest.mark.parametrize("seed", range(10))
def test_volume_derivation_matches_each_whatif_flattened_by_itself(seed):
    """`check_whatif_derivation(volumes=True)`: every staying node's counts, limits and multi-claim set, and the volume test of every batch pod on every staying
    node, against the what-if flattened by itself -- 42 candidate sets per snapshot, 420 pairs in all."""
    rs = np.random.RandomState(40 + seed)
    spec = ["topology" if seed == 9 else "plain", int(rs.randint(24, 80)), int(rs.randint(4, 8)), 600 + seed]
    snap, pod_node, bound = build_case(spec)
    parsed = S.ParsedProblem(snap)
    n = len(snap.nodes)
    sets = [[int(x) for x in rs.choice(n, size=int(rs.choice([1, 1, 2, 3, 6, 12])), replace=False)] for _ in range(36)]
    sets += [[n - 1], list(range(n // 2)), list(range(n)), [], [0, n - 1], list(range(n - 1, 0, -3))]
    for cs in sets:
        S.check_whatif_derivation(parsed, pod_node, cs, volumes=True)
    parsed.close()


def test_claims_listed_on_nodes_that_no_pod_mounts():
    """Without the flag the restatement refuses the snapshot (the flag-0 partition depends on the candidate set); with it, claims a node lists but no bound pod
    mounts -- one of them on two nodes -- only count on their nodes, and the derivation still matches every what-if flattened by itself."""
    snap, pod_node, bound = build_case(["plain", 30, 5, 9])
    parsed = S.ParsedProblem(snap)
    with pytest.raises(S.KSolveError) as e:
        S.check_whatif_derivation(parsed, pod_node, [0])
    assert e.value.code == S.KS_ERR_UNSUPPORTED and "volume" in str(e.value)
    S.check_whatif_derivation(parsed, pod_node, [0], volumes=True)
    parsed.close()
    from karpenter_core_amd.model import Volume
    snap.nodes[1].volumes = snap.nodes[1].volumes + [Volume(W.EBS_DRIVER, "default/unmounted-a"), Volume(W.EBS_DRIVER, "default/unmounted-b")]
    snap.nodes[2].volumes = snap.nodes[2].volumes + [Volume(W.EBS_DRIVER, "default/unmounted-a")]
    parsed = S.ParsedProblem(snap)
    for cs in ([0], [1], [2, 3], list(range(10))):
        S.check_whatif_derivation(parsed, pod_node, cs, volumes=True)
    parsed.close()


def test_volume_snapshots_keep_their_refusal_without_the_flag():
    """flags = 0 refuses as before; with the flag the same snapshot is derivable (the device part is checked under `-m gpu`)."""
    snap, pod_node, bound = build_case(["plain", 24, 4, 5])
    parsed = S.ParsedProblem(snap)
    with pytest.raises(S.KSolveError) as e:
        S.check_whatif_derivation(parsed, pod_node, [0, 1])
    assert "the shared-claim partition depends on the candidate set" in str(e.value)
    S.check_whatif_derivation(parsed, pod_node, [0, 1], volumes=True)
    parsed.close()


def test_more_than_64_limited_drivers_are_still_refused():
    """What the flag cannot derive is refused with a message; open_whatifs(derive=None) then flattens on the host as today."""
    snap, pod_node, bound = build_case(["plain", 24, 4, 6])
    snap.nodes[0].volume_limits = dict(snap.nodes[0].volume_limits, **{f"driver-{k}.csi": 5 for k in range(70)})
    parsed = S.ParsedProblem(snap)
    with pytest.raises(S.KSolveError) as e:
        S.check_whatif_derivation(parsed, pod_node, [1], volumes=True)
    assert e.value.code == S.KS_ERR_UNSUPPORTED and "64" in str(e.value)
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- CPU: flag 0 unchanged
def test_flag0_flattening_of_volume_snapshots_is_unchanged():
    """tests/golden/volume_fingerprints.json was made before the flag existed: the snapshot's flag-0 flattening and the what-ifs flattened over it are the same
    bytes, and the flagged flattening is a different one."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_volume_fingerprints as G
    want = json.load(open(os.path.join(HERE, "golden", "volume_fingerprints.json")))
    assert G.compute() == want
    existing, sizes, seed = G.CASES["vol-48x5-s1"]
    snap, pod_node = W.snapshot_problem(*W.volume_snapshot(existing, sizes, seed), True)
    parsed = S.ParsedProblem(snap)
    flagged = parsed.snapshot_fingerprint(pod_node, volumes=True)
    assert "%016x" % parsed.snapshot_fingerprint(pod_node) == want["vol-48x5-s1/snapshot"] != "%016x" % flagged
    assert parsed.snapshot_fingerprint(pod_node, cold=True, volumes=True) == flagged
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- CPU: events
def flat_hashes(parsed, pod_node, sets):
    flats = S.open_whatifs(parsed, pod_node, sets, derive=False)
    out = [f.fingerprint() for f in flats]
    for f in flats:
        f.close()
    return out


def cluster_after_with_volumes(nodes, bound, events):
    """`workloads.cluster_after`, with each node's volume usage following its pods (one entry per pod that mounts a claim, as state/node.go keeps it)."""
    nodes, bound, slot = W.cluster_after(nodes, bound, events)
    for n, b in zip(nodes, bound):
        n.volumes = [v for p in b for v in p.volumes]
    return nodes, bound, slot


def volume_pod(rs, uid, shared):
    """A generic pod with a private claim, one of the cluster's RWX claims, a claim of the unlimited driver, or none."""
    from karpenter_core_amd.model import Volume
    p = W.generic_pod(rs, uid)
    r = rs.rand()
    if r < 0.4:
        p.volumes = [Volume(W.EBS_DRIVER, f"default/data-{uid}")]
    elif r < 0.7:
        p.volumes = [Volume(W.EFS_DRIVER, shared[int(rs.randint(len(shared)))])]
    elif r < 0.8:
        p.volumes = [Volume(W.FSX_DRIVER, "default/scratch-0000")]
    return p


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_events_keep_the_flagged_flattening_equal_to_a_fresh_one(seed):
    """BIND / UNBIND / NODE+ / NODE- of pods and nodes with claims through `ParsedProblem.apply`: after every batch the flagged flattening equals one made from
    scratch over the same objects, and the derivation restatement holds on it and on a snapshot ingested afresh from the cluster as it is now (each equal to
    its what-ifs flattened by themselves; after the first batch, which only adds, those what-ifs are array for array the same on both)."""
    rs = np.random.RandomState(seed)
    its, prov, nodes, bound = W.volume_snapshot(36, 6, 700 + seed, unowned=False)
    shared = sorted({v.pvc_id for b in bound for p in b for v in p.volumes if "rwx" in v.pvc_id}) or ["default/rwx-0000"]
    snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
    parsed = S.ParsedProblem(snap)
    S.check_whatif_derivation(parsed, pn, [0], volumes=True)      # (the flagged flattening exists before the first event: the events continue it)
    first = True
    for batch in range(8):
        events = []
        for k in range(int(rs.randint(1, 6))):
            cur_nodes, cur_bound, _ = cluster_after_with_volumes(nodes, bound, events)
            kind = rs.choice(["node+", "bind", "bind", "bind", "unbind", "unbind", "node-"] if batch % 2 else ["node+", "bind", "bind"])
            if kind == "node+":
                n = W.fresh_node(its, f"s{seed}b{batch}-node-{k}", rs)
                n.volume_limits = {W.EBS_DRIVER: int(rs.choice([2, 3, 25]))}
                events.append(("node+", n))
            elif kind == "node-" and len(cur_nodes) > 6:
                events.append(("node-", cur_nodes[int(rs.randint(len(cur_nodes)))].name))
            elif kind == "unbind" and any(cur_bound):
                i = int(rs.choice([j for j, b in enumerate(cur_bound) if b]))
                events.append(("unbind", cur_bound[i][int(rs.randint(len(cur_bound[i])))].uid))
            else:
                events.append(("bind", cur_nodes[int(rs.randint(len(cur_nodes)))].name, volume_pod(rs, f"s{seed}b{batch}-pod-{k}", shared)))
        nodes, bound, slot = cluster_after_with_volumes(nodes, bound, events)
        info = parsed.apply(events, pn if first else None)
        first = False
        assert info["applied"] == len(events)
        assert parsed.snapshot_fingerprint(volumes=True) == parsed.snapshot_fingerprint(cold=True, volumes=True), f"batch {batch}"
        bind, _ = parsed.bindings()
        fresh, fresh_pn = W.snapshot_problem(its, prov, nodes, bound, False)
        fresh_parsed = S.ParsedProblem(fresh)
        live = [i for i in range(len(nodes)) if bound[i]]
        for cs in ([live[0]], live[: len(live) // 2], [live[-1], live[0]], []):
            S.check_whatif_derivation(parsed, None, [slot[i] for i in cs], volumes=True)
            S.check_whatif_derivation(fresh_parsed, fresh_pn, cs, volumes=True)
        if batch == 0:      # adds only: the what-ifs over the patched snapshot are, array for array, the ones over the fresh snapshot
            sets = [[slot[i]] for i in live[:6]] + [[slot[i] for i in live[:9]]]
            assert flat_hashes(parsed, None, sets) == flat_hashes(fresh_parsed, fresh_pn, [[live[i]] for i in range(6)] + [live[:9]])
        fresh_parsed.close()
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_config4_shape_volume_whatifs_match_host_records_and_price_stage(tmp_path):
    """512 config-#4 what-ifs over a 2 048-node `volume_snapshot`: derived with volumes == flattened on the host, record for record (result_records), and the
    price stage (launch_pick, price_filter at the pick's price) reads the same from both."""
    import torch
    its, prov, nodes, bound = W.volume_snapshot(2048, 50, 45)
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
    sets = W.config4_sets(512, 2048, 45)
    parsed = S.ParsedProblem(snap)
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True, volumes=True)
    flat = S.open_whatifs(parsed, pod_node, sets, derive=False)
    try:
        words = (len(its) + 63) // 64
        S.solve_batch_resident(derived)
        S.solve_batch(flat, decode=False)
        rec = torch.zeros((len(sets), 3 + words), dtype=torch.int64, device="cuda:0")
        S.result_records_dev(derived, list(range(len(sets))), words, rec)
        want = S.result_records(flat, list(range(len(sets))), words)
        assert (rec.cpu().numpy() == want).all()
        with_node = [i for i in range(len(sets)) if want[i][1] > 0]
        if with_node:
            d, h, zero = [derived[i] for i in with_node], [flat[i] for i in with_node], [0] * len(with_node)
            picks = S.launch_pick(d, zero)
            assert picks == S.launch_pick(h, zero)
            ceiling = [p[3] if p else 0.0 for p in picks]
            assert S.price_filter(d, zero, ceiling) == S.price_filter(h, zero, ceiling)
    finally:
        for f in derived + flat:
            f.close()
        parsed.close()


@pytest.mark.gpu
def test_a_batch_of_one_volume_whatif_and_the_oracle():
    """One what-if: the multi-wave kernel, with the what-if's own volume state."""
    from oracle import oracle_py as O
    snap, pod_node, bound = build_case(["plain", 48, 6, 21])
    cs = [3, 9, 11, 20, 30]
    parsed = S.ParsedProblem(snap)
    (f,) = S.open_whatifs(parsed, pod_node, [cs], derive=True, volumes=True)
    try:
        got = f.solve()
        want = O.solve(whatif_problem(snap, bound, cs))
        assert got.canonical() == want.canonical() and got.reasons == want.reasons
    finally:
        f.close()
        parsed.close()


@pytest.mark.gpu
def test_volume_state_is_initialised_under_a_poisoned_arena(tmp_path):
    """KS_POISON=0xFF fills the what-ifs' uninitialised region -- where each what-if's volume counts and sets live -- before the solve: results are unchanged."""
    jobs = {name: job for name, job in all_jobs().items() if name in ("vol-3", "vol-11", "wide-14", "topology")}
    res = run_in_child(jobs, bool(os.environ.get("KS_TEST_SIM")), str(tmp_path), {"KS_POISON": "0xFF"})
    for name in jobs:
        check_case(res, name)
