"""Derived what-ifs whose per-node topology facts are held as LISTS PER NODE (kshost.h KSH_DERIVE_GROUP_LISTS, ksolve.h ks_whatif_topo_lists /
ks_whatifs_open_lists, csrc/ksolve.hip ks_derive_topology_lists): any number of topology groups, where the dense tables stop at 1 024.

  CPU  -- a 24-node snapshot whose 1 040 two-pod applications each own their groups (G > 1024): `ksh_check_whatif_derivation` with the flag restates the
          derivation from the lists and holds it against every what-if flattened by itself; without the flag the snapshot is refused as before.  The same check
          over the random clusters of tests/test_whatif_derived.py, and what the flag must not move (the flag-0 fingerprint).
  GPU  -- below the cap the two routes agree cell by cell (`ksh_debug_whatif_topology`) and result text by result text; above it the derived what-ifs equal the ones
          flattened on the host and the oracle, every handle is a derived one (its arena is not empty), and `ksh_consolidation_commands` returns the fallback's rows.
  C    -- tests/cabi_usage_group_lists.c as C99, on the emulator build and on the device."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import scheduler as S, workloads as W
from karpenter_core_amd.model import (ClusterPod, Container, DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_ZONE, LabelSelector, Pod, PodAffinityTerm, StateNode,
                                      TopologySpreadConstraint)
from test_whatif_derived import _topology_snapshot, _whatif_problem

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

APPS_ABOVE, APPS_AT_CAP = 1040, 819      # 5 groups per 4 applications (the anti-affinity owns its group and the inverse one): 1 300 groups; 819 applications: exactly 1 024


def many_groups_cluster(apps, owned=23):
    """`owned` (23) owned nodes in 3 zones and one node no provisioner owns; `apps` two-pod applications, each selecting only itself.  By i % 4: zonal spread, hostname spread,
    required hostname anti-affinity, zonal pod affinity -- no pod is selected by more than its own groups.  A few pods that are in no batch (daemon-like) count under
    some applications' labels, on owned nodes and on the unowned one."""
    its, prov, nodes, _ = W.cluster_snapshot(owned, 5, 8)
    zones = sorted({n.labels[LABEL_ZONE] for n in nodes})
    assert len(zones) == 3
    bound = [[] for _ in nodes]
    for i in range(apps):
        own = LabelSelector({"app": f"app-{i:04d}"})
        a = i % owned
        for k, nd in enumerate((a, (a + 1 + i % 7) % owned)):      # (two different nodes: the anti-affinity holds in the snapshot)
            p = Pod(uid=f"app-{i:04d}-{k}", labels={"app": f"app-{i:04d}"}, containers=[Container(requests={"cpu": "10m", "memory": "10Mi"})])
            if i % 4 == 0:
                p.spread = [TopologySpreadConstraint(1, LABEL_ZONE, DO_NOT_SCHEDULE, own)]
            elif i % 4 == 1:
                p.spread = [TopologySpreadConstraint(2, LABEL_HOSTNAME, DO_NOT_SCHEDULE, own)]
            elif i % 4 == 2:
                p.anti_required = [PodAffinityTerm(LABEL_HOSTNAME, own)]
            else:
                p.affinity_required = [PodAffinityTerm(LABEL_ZONE, own)]
            bound[nd].append(p)
    nodes.append(StateNode(name="unowned", labels={LABEL_ZONE: zones[0], LABEL_HOSTNAME: "unowned"}))
    bound.append([dataclasses.replace(p, uid=f"extra-{j}") for j, p in enumerate(bound[0][:8])])
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, True)
    for j in range(40):      # pods that are in no batch: they keep counting while their node stays -- and, under a hostname, after it has left
        snap.cluster_pods.append(ClusterPod(uid=f"ds-{j}", namespace="default", node_name=nodes[(j * 5) % len(nodes)].name, labels={"app": f"app-{(j * 3) % apps:04d}"}))
    return its, prov, nodes, bound, snap, pod_node


_CLUSTERS = {}


def cluster(apps):
    if apps not in _CLUSTERS:
        _CLUSTERS[apps] = many_groups_cluster(apps)
    return _CLUSTERS[apps]


def candidate_sets(nodes):
    zone0 = [i for i, n in enumerate(nodes) if n.labels[LABEL_ZONE] == nodes[0].labels[LABEL_ZONE] and n.name != "unowned"]
    return {"empty": [], "one": [5], "a zone": zone0, "with the unowned node": [2, len(nodes) - 1, 11]}


def groups_of(snap):
    f = S.FlatProblem(snap)
    try:
        return f.dims["G"]
    finally:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_above_1024_groups_the_lists_derive_and_the_tables_refuse():
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_ABOVE)
    G = groups_of(snap)
    GW = (G + 63) // 64
    assert G > 1024 and GW & (GW - 1), (G, GW)      # (the owner words of the dense form would not be a power of two)
    parsed = S.ParsedProblem(snap)
    for name, cs in candidate_sets(nodes).items():
        with pytest.raises(S.KSolveError) as e:
            S.check_whatif_derivation(parsed, pod_node, cs)
        assert e.value.code == S.KS_ERR_UNSUPPORTED and "more than 1024 topology groups" in str(e.value), name
        S.check_whatif_derivation(parsed, pod_node, cs, group_lists=True)
    # events unbind pods -- of every kind of application, one of them the only pod of its application on its node -- so that tombstones exist; the lists are
    # rebuilt with the flattening the library keeps (the flag-on one: the last call used it)
    gone = [bound[3][0].uid, bound[3][1].uid, bound[3][2].uid, bound[3][3].uid, bound[9][0].uid, bound[len(nodes) - 1][0].uid]
    info = parsed.apply_block([("unbind", u) for u in gone], pod_node)
    assert info["applied"] == len(gone)
    now, _ = parsed.bindings()
    assert (now < 0).sum() == len(gone)
    for cs in ([3], [3, 9, len(nodes) - 1], [0, 1, 2, 3, 4]):
        S.check_whatif_derivation(parsed, None, cs, group_lists=True)
        with pytest.raises(S.KSolveError) as e:
            S.check_whatif_derivation(parsed, None, cs)
        assert e.value.code == S.KS_ERR_UNSUPPORTED
    assert parsed.snapshot_fingerprint(None, group_lists=True) == parsed.snapshot_fingerprint(None, cold=True, group_lists=True)      # continued == from scratch, lists included
    parsed.close()


def test_without_a_device_the_flag_on_route_is_eligible_and_the_flag_off_one_is_not():
    """`open_whatifs(derive=True)`: without the flag the snapshot is refused on the host (KS_ERR_UNSUPPORTED, the cap); with it the host has nothing to object --
    what stops the call on a machine without a GPU is the missing device."""
    if S.device_count() > 0:
        pytest.skip("GPU present")
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_ABOVE)
    parsed = S.ParsedProblem(snap)
    with pytest.raises(S.KSolveError) as e:
        S.open_whatifs(parsed, pod_node, [[0]], derive=True)
    assert e.value.code == S.KS_ERR_UNSUPPORTED and "1024" in str(e.value)
    with pytest.raises(S.KSolveError) as e:
        S.open_whatifs(parsed, pod_node, [[0]], derive=True, group_lists=True)
    assert e.value.code == S.KS_ERR_DEVICE
    parsed.close()


@pytest.mark.parametrize("seed", range(6))
def test_the_lists_derive_what_the_tables_derive_on_random_clusters(seed):
    """The clusters of tests/test_whatif_derived.py (spread, affinity, preferred terms, required anti-affinity per hostname and per zone, pods in no batch, a node
    nobody knows, an unowned node): the derivation restated from the lists equals every what-if flattened by itself, as the one restated from the tables does."""
    rs = np.random.RandomState(500 + seed)
    its, prov, nodes, bound, snap, pod_node = _topology_snapshot(int(rs.randint(24, 90)), int(rs.randint(4, 8)), 300 + seed, spare=int(rs.choice([-1, 0, 3])),
                                                                  extras=seed % 4 != 0, anti=seed % 3 != 0, wide=seed % 5 == 4)
    parsed = S.ParsedProblem(snap)
    sets = [[int(x) for x in rs.choice(len(nodes), size=int(rs.choice([1, 1, 2, 4, 9, 20])), replace=False)] for _ in range(20)] + [[], [len(nodes) - 1], list(range(len(nodes)))[:30]]
    for cs in sets:
        S.check_whatif_derivation(parsed, pod_node, cs, group_lists=True)
        S.check_whatif_derivation(parsed, pod_node, cs)
    parsed.close()


def test_the_flag_moves_no_flag_off_fingerprint_and_names_no_kernel_flag():
    its, prov, nodes, bound, snap, pod_node = _topology_snapshot(40, 6, 7, spare=-1, anti=True)
    fresh = S.ParsedProblem(snap)
    want = fresh.snapshot_fingerprint(pod_node)
    used = S.ParsedProblem(snap)
    S.check_whatif_derivation(used, pod_node, [0, 1, 2], group_lists=True)
    on = used.snapshot_fingerprint(pod_node, group_lists=True)
    assert used.snapshot_fingerprint(pod_node) == want and used.snapshot_fingerprint(pod_node, cold=True) == want
    assert on == used.snapshot_fingerprint(pod_node, cold=True, group_lists=True) and on != want      # (its own flattening, kept apart: it hashes the lists)
    assert S.KSH_DERIVE_GROUP_LISTS == 1 << 18
    assert not S.KSH_DERIVE_GROUP_LISTS & (S.KS_FLAG_SIMULATION | S.KS_FLAG_STATS | S.KS_FLAG_NO_RR | S.KS_FLAG_ONE_WAVE | S.KS_FLAG_NO_LEAN | S.KSH_DERIVE_VOLUMES | S.KSH_ACTIVE_RESOURCES)
    for p in (fresh, used):
        p.close()


def test_the_refusals_of_the_dense_route_stay_under_the_flag():
    """One spread group shared by pods whose node filters differ: refused with the flag as without it."""
    from test_whatif_derived import _snapshot
    its, prov, nodes, bound = _snapshot(24, 5, 8)
    zones = sorted({n.labels[LABEL_ZONE] for n in nodes})
    for i, pods in enumerate([b for b in bound if b][:6]):
        pods[0].labels = {"my-label": "a"}
        pods[0].node_selector = {LABEL_ZONE: zones[i % len(zones)]}
        pods[0].spread = [TopologySpreadConstraint(2, LABEL_HOSTNAME, DO_NOT_SCHEDULE, LabelSelector({"my-label": "a"}))]
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, True)
    parsed = S.ParsedProblem(snap)
    with pytest.raises(S.KSolveError) as e:
        S.check_whatif_derivation(parsed, pod_node, [0], group_lists=True)
    assert e.value.code == S.KS_ERR_UNSUPPORTED and "node filters differ" in str(e.value)
    parsed.close()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _solve_texts(flats):
    """ksh_solve_batch, the KSR1 text of every result as the library wrote it (ksh_result_text's) -- without its STATS line, which holds clock readings of the run
    (cycle counters, solve_ns) and no part of the result: new nodes, placements, requirements, stages and reasons are all compared byte for byte."""
    kh = S.libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    outs = (ctypes.c_void_p * n)()
    kms, wms = ctypes.c_float(), ctypes.c_double()
    rc = kh.ksh_solve_batch(hs, n, outs, ctypes.byref(kms), ctypes.byref(wms))
    if rc != S.KS_OK:
        raise S.KSolveError(rc, kh.ksh_last_error().decode())
    texts = []
    for i in range(n):
        lines = ctypes.string_at(outs[i]).split(b"\n")
        assert sum(l.startswith(b"STATS ") for l in lines) == 1 and lines[0] == b"KSR1"
        texts.append(b"\n".join(l for l in lines if not l.startswith(b"STATS ")))
        kh.ksh_free(outs[i])
    return texts


def _routes_agree(snap, pod_node, sets, tag):
    parsed = S.ParsedProblem(snap)
    dense = S.open_whatifs(parsed, pod_node, sets, derive=True)
    lists = S.open_whatifs(parsed, pod_node, sets, derive=True, group_lists=True)
    try:
        assert all(f.arena_bytes() for f in dense + lists)
        for i, (a, b) in enumerate(zip(dense, lists)):
            for what, x, y in zip(("active", "count", "extra"), a.whatif_topology(), b.whatif_topology()):
                assert x.shape == y.shape and (x == y).all(), (tag, i, sets[i], what, np.argwhere(x != y)[:5].tolist())
        for i, (x, y) in enumerate(zip(_solve_texts(dense), _solve_texts(lists))):
            assert x == y, (tag, i, sets[i])
    finally:
        for f in dense + lists:
            f.close()
        parsed.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,seed", [("topology", 0), ("topology", 3), ("anti", 1), ("anti", 4), ("wide", 2)])
def test_below_the_cap_the_two_routes_agree_cell_by_cell(kind, seed):
    """The clusters of the derived-what-if tests -- spread, affinity, inverse anti-affinity, unowned nodes -- opened with and without the flag: the same group
    activity, domain counts and hostname extras in every what-if, and the same result text."""
    rs = np.random.RandomState({"topology": 0, "anti": 100, "wide": 200}[kind] + seed)
    if kind == "topology":
        c = _topology_snapshot(int(rs.randint(24, 120)), int(rs.randint(4, 8)), 50 + seed, spare=int(rs.choice([-1, 0, 3])), extras=seed != 0)
    elif kind == "anti":
        c = _topology_snapshot(int(rs.randint(24, 100)), int(rs.randint(4, 8)), 150 + seed, spare=int(rs.choice([-1, 0, 3])), extras=seed != 0, anti=True)
    else:
        c = _topology_snapshot(int(rs.randint(60, 120)), int(rs.randint(4, 8)), 250 + seed, spare=int(rs.choice([-1, 3])), anti=True, wide=True)
    its, prov, nodes, bound, snap, pod_node = c
    sets = [[int(x) for x in rs.choice(len(nodes), size=int(rs.choice([1, 1, 2, 4, 9])), replace=False)] for _ in range(20)] + [[len(nodes) - 1], [0, len(nodes) - 1], list(range(min(len(nodes), 300)))]
    _routes_agree(snap, pod_node, sets, (kind, seed))


@pytest.mark.gpu
def test_at_exactly_1024_groups_the_two_routes_agree_cell_by_cell():
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_AT_CAP)
    assert groups_of(snap) == 1024
    sets = list(candidate_sets(nodes).values())[1:] + [[i] for i in (0, 7, 22)] + [list(range(len(nodes)))]
    _routes_agree(snap, pod_node, sets, "1024")


@pytest.mark.gpu
@pytest.mark.parametrize("group_lists", [False, True])
def test_more_than_256_hostname_keyed_groups_solve_like_flattened(group_lists):
    """The 1 024-group snapshot holds 615 hostname-keyed groups.  A derived what-if runs on the SNAPSHOT's class plans, whose hostname items name a row of the hostname
    tables: the row is held in full (PlanTopo::hrow), not in 8 bits -- on either route the what-ifs solve like the ones flattened by themselves (a handful of groups each)."""
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_AT_CAP)
    sets = _sixteen_sets(nodes)
    parsed = S.ParsedProblem(snap)
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True, group_lists=group_lists)
    flat = S.open_whatifs(parsed, pod_node, sets, derive=False)
    try:
        assert derived[0].dims["GH"] > 256 and all(f.arena_bytes() for f in derived)
        got, _, _ = S.solve_batch(derived)
        want, _, _ = S.solve_batch(flat)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.canonical() == b.canonical() and a.reasons == b.reasons, (group_lists, i, sets[i])
    finally:
        for f in derived + flat:
            f.close()
        parsed.close()


def _sixteen_sets(nodes):
    rs = np.random.RandomState(16)
    return list(candidate_sets(nodes).values())[1:] + [[int(x) for x in rs.choice(len(nodes), size=int(rs.choice([1, 2, 3, 5])), replace=False)] for _ in range(13)]


@pytest.mark.gpu
def test_above_the_cap_derived_equals_flattened_and_the_oracle():
    """1 300 groups, 16 candidate sets: every what-if derived under the flag solves like the same what-if flattened on the host and like the oracle.  Every handle is
    a derived one -- its batch's arena is not empty: a silent fall-back to host flattening would show here."""
    from oracle import oracle_py as O
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_ABOVE)
    sets = _sixteen_sets(nodes)
    assert len(sets) == 16
    parsed = S.ParsedProblem(snap)
    with pytest.raises(S.KSolveError) as e:
        S.open_whatifs(parsed, pod_node, sets, derive=True)
    assert e.value.code == S.KS_ERR_UNSUPPORTED and "1024" in str(e.value)
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True, group_lists=True)
    flat = S.open_whatifs(parsed, pod_node, sets, derive=False)
    try:
        assert all(f.arena_bytes() != 0 for f in derived) and not any(f.arena_bytes() for f in flat)
        got, _, _ = S.solve_batch(derived)
        want, _, _ = S.solve_batch(flat)
        for i, (a, b) in enumerate(zip(got, want)):
            assert a.canonical() == b.canonical() and a.reasons == b.reasons, (i, sets[i])
            ref = O.solve(_whatif_problem(snap, pod_node, sets[i]))
            assert a.canonical() == ref.canonical(), (i, sets[i])
    finally:
        for f in derived + flat:
            f.close()
        parsed.close()


@pytest.mark.gpu
def test_above_the_cap_the_commands_are_the_fallback_routes():
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_ABOVE)
    sets = [cs for cs in _sixteen_sets(nodes) if len(nodes) - 1 not in cs]      # (an unowned node is no consolidation candidate)
    words = (len(its) + 63) // 64
    parsed = S.ParsedProblem(snap)
    try:
        want, _ = S.consolidation_commands(parsed, pod_node, sets, words)
        got, _ = S.consolidation_commands(parsed, pod_node, sets, words, flags=S.KSH_DERIVE_GROUP_LISTS)
        assert (got == want).all(), np.argwhere(got != want)[:8].tolist()
    finally:
        parsed.close()


# ---------------------------------------------------------------------------------------------------------------- the C ABI from C
def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_group_lists")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_group_lists.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    its, prov, nodes, bound, snap, pod_node = cluster(APPS_ABOVE)
    f = tmp_path / "snapshot.ksp"
    f.write_text(snap.to_ksp())
    out = subprocess.run([exe, str(f)] + [str(int(x)) for x in pod_node], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert any(l.startswith("refused: ") and "1024" in l for l in lines), out.stdout
    G = groups_of(snap)
    assert f"groups: {G}" in lines, out.stdout
    rows = [l for l in lines if l.startswith("what-if ")]
    assert len(rows) == 3 and all("arena 0 bytes" not in l for l in rows), out.stdout
    # what-if 0 removes node 0: active are the groups its pods own -- one per application with a pod there -- and the inverse groups, which exist in every what-if
    assert f" active {len({p.labels['app'] for p in bound[0]}) + APPS_ABOVE // 4} of {G} groups" in rows[0], rows[0]


def test_c_abi_from_c_on_the_emulator(tmp_path):
    """tests/cabi_usage_group_lists.c as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries."""
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_c_abi_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
