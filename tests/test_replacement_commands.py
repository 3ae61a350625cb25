"""Expiration / Drift.ComputeCommand with m -> n rows through the C ABI (include/kshost.h ksh_replacement_commands / ksh_replacement_option; kernels ks_replacement_heads /
ks_replacement_nodes in csrc/ksolve.hip) against tests/deprovisioning_ref.py over oracle/consolidation_ref.py's simulation.  As in tests/test_validate_commands.py every
case runs unmarked on the emulator in a child process and marked `gpu` on the device; the comparisons happen here; the clusters come from tests/test_consolidation.py and
tests/test_consolidation_commands.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import fake
from karpenter_core_amd.model import Container, Offering, Pod
from oracle import consolidation_ref as CR

import deprovisioning_ref as D
import test_consolidation as TC
import test_consolidation_commands as CC
import test_deprovisioning_ref as TDR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POISON = 0xA5A5A5A5A5A5A5A5
SCAN_TILE = 256      # KS_REP_TILE of csrc/ksolve.hip


def _t71():
    """71 instance types; the pod (2 cpu) fits only the last seven, so every option bit is in the SECOND word."""
    cur = fake.new_instance_type("current", {"cpu": "4"}, offerings=[Offering("on-demand", "test-zone-1a", 0.5, False)])
    its = [cur] + [fake.new_instance_type(f"t{i:02d}", {"cpu": "1" if i < 64 else "4"}, offerings=[Offering("on-demand", "test-zone-1a", 0.1 + i / 100)]) for i in range(1, 71)]
    return TC.snapshot(its, [TC.node("n1", cur, "on-demand", "test-zone-1a", cpu="4")], [[TC.pod("p1", "2")]])


def _active12():
    """A 12-name catalogue of which the pods request four: under KSH_ACTIVE_RESOURCES the request words and ksh_snapshot_name(what = 2) speak of the active names."""
    res = {"cpu": "8", "memory": "16Gi", "pods": "32"}
    res.update({f"example.com/r{i}": "4" for i in range(9)})
    cur = fake.new_instance_type("current", res, offerings=[Offering("on-demand", "test-zone-1a", 0.5, False)])
    rep = fake.new_instance_type("replacement", res, offerings=[Offering("on-demand", "test-zone-1a", 0.3)])
    p = Pod(uid="p1", labels={"app": "test"}, containers=[Container(requests={"cpu": "1", "example.com/r5": "2"})])
    return TC.snapshot([cur, rep], [TC.node("n1", cur, "on-demand", "test-zone-1a", cpu="8")], [[p]])


def _handmade_deleting():
    snap = CC._handmade()
    snap.deleting = (2,)
    return snap


_BUILT = {}


def case(name):
    """-> (snapshot, candidate sets, active_resources)"""
    if name not in _BUILT:
        if name.startswith("rep-"):
            snap, cands, _, _ = TC.replacement_scenarios()[name[4:]]
            out = (snap, [[c] for c in cands], False)
        elif name == "handmade":                 # [3]: two new nodes; [4]: a pod that fits nothing -> n_unscheduled > 0 and still a command
            out = (CC._handmade(), [[0], [1], [2], [3], [4], [0, 1], [3, 4]], False)
        elif name == "deleting_between":         # an error head with n_nodes = 0 between two sets with n_nodes > 0: the offsets
            out = (_handmade_deleting(), [[3], [2], [0], [1, 2], [4]], False)
        elif name == "uninitialised":            # delete with the blocked flag, where consolidation.replacement_command says replace
            out = (TDR._uninitialised_neighbour_that_cannot_help(), [[0]], False)
        elif name == "delete_between":           # a plain delete (n_nodes = 0) between two replaces
            snap, _, _ = TC.scenarios()["can_delete_nodes"]
            out = (snap, [[0, 1], [0], [0, 1]], False)
        elif name == "t71":
            out = (_t71(), [[0]], False)
        elif name == "active12":
            out = (_active12(), [[0]], True)
        elif name == "scan":                     # one scan tile plus three sets, repeating: the carry
            out = (CC._handmade(), ([[3], [0], [4], [1], [2]] * 60)[:SCAN_TILE + 3], False)
        else:
            raise KeyError(name)
        _BUILT[name] = out
    return _BUILT[name]


CASES = ["rep-delete_empty", "rep-replace_one", "rep-replace_with_three", "rep-first_candidate_only", "handmade", "deleting_between", "uninitialised", "delete_between", "t71", "active12", "scan"]


# ---------------------------------------------------------------------------------------------------------------- the reference
def ref_set(snap, cs):
    deleting = set(int(j) for j in getattr(snap, "deleting", ()))
    if set(cs) & deleting:
        return {"action": "error", "why": 10, "blocked": False, "n_new": 0, "n_unscheduled": 0, "nodes": []}
    sink = []
    CR.compute_consolidation(snap, list(cs), sink)
    res = sink[0]
    blocked = any(j not in cs and j not in deleting and n.in_state and n.owned and n.labels.get("karpenter.sh/initialized") != "true" for j, n in enumerate(snap.nodes))
    new = [] if blocked else res.new_nodes      # helpers.go:106-113: `return nil, false, nil`
    return {"action": "replace" if new else "delete", "why": 0, "blocked": blocked, "n_new": len(res.new_nodes), "n_unscheduled": len(res.unscheduled),
            "nodes": [{"options": sorted(n.instance_types), "requirements": _reqs(n), "requests": dict(n.requests)} for n in new]}


def _reqs(n):
    return {k: [v[0], list(v[1]), v[2], v[3]] for k, v in CR.canon_reqs(dict(n.requirements)).items()}


_REF = {}


def ref(name):
    if name not in _REF:
        snap, sets, _ = case(name)
        memo = {}
        _REF[name] = [memo.setdefault(tuple(cs), ref_set(snap, cs)) for cs in sets]
    return _REF[name]


# ---------------------------------------------------------------------------------------------------------------- the device side
ACTIONS = {0: "do-nothing", 1: "delete", 2: "replace", 3: "error"}


def _decode(S, snap, parsed, heads, nodes, words):
    out = []
    for h in heads:
        d = S.decode_replacement_head(h)
        d["action"] = ACTIONS[d["action"]]
        d["nodes"] = []
        if not d["truncated"]:
            for row in nodes[d["node_off"]:d["node_off"] + d["n_nodes"]] if d["n_nodes"] else []:
                nd = S.decode_replacement_node(parsed, row, words)
                nd["options"] = sorted(snap.instance_types[t].name for t in nd["options"])
                nd["requirements"] = {k: [v[0], list(v[1]), v[2], v[3]] for k, v in nd["requirements"].items()}
                d["nodes"].append(nd)
        out.append(d)
    return out


def device_run(S, name):
    from karpenter_core_amd import consolidation as C
    if name == "option":
        return option_run(S)
    snap, sets, active = case(name)
    parsed, pod_node, leaving = C._command_snapshot(snap)
    try:
        TW = (len(snap.instance_types) + 63) // 64
        n = len(sets)
        out = {}
        # the sizing call, then a table exactly large enough
        h0 = np.full((n, S.KS_REP_HEAD_WORDS), POISON, dtype=np.uint64)
        _, _, total, _ = S.replacement_commands(parsed, pod_node, sets, TW, cap_nodes=0, deleting=leaving, active_resources=active, heads=h0)
        out["total"] = total
        out["sizing"] = _decode(S, snap, parsed, h0, None, TW) if total == 0 else [S.decode_replacement_head(h) for h in h0]
        heads, nodes, total2, ms = S.replacement_commands(parsed, pod_node, sets, TW, cap_nodes=total, deleting=leaving, active_resources=active)
        out["exact"] = _decode(S, snap, parsed, heads, nodes, TW)
        out["total_exact"], out["ms"] = total2, ms
        # hygiene: poisoned tables two words wider than needed and two rows longer; every word written, surplus and reserved words zero, rows otherwise identical
        W2 = TW + 2
        hp = np.full((n, S.KS_REP_HEAD_WORDS), POISON, dtype=np.uint64)
        npz = np.full((total + 2, S.replacement_node_words(W2)), POISON, dtype=np.uint64)
        S.replacement_commands(parsed, pod_node, sets, W2, cap_nodes=total + 2, deleting=leaving, active_resources=active, heads=hp, nodes=npz)
        base = S.KS_REP_NODE_OPTIONS
        out["hygiene"] = {"heads_equal": bool((hp == heads).all()), "no_poison": bool((hp != POISON).all()) and bool((npz[:total] != POISON).all()),
                          "surplus_zero": bool((npz[:total, base + TW:] == 0).all()), "rows_equal": bool((npz[:total, :base + TW] == nodes[:total]).all()) if total else True,
                          "beyond_intact": bool((npz[total:] == POISON).all())}
        # one row short
        if total:
            cap = total - 1
            hs = np.full((n, S.KS_REP_HEAD_WORDS), POISON, dtype=np.uint64)
            ns = np.full((total + 1, S.replacement_node_words(TW)), POISON, dtype=np.uint64)
            _, _, total3, _ = S.replacement_commands(parsed, pod_node, sets, TW, cap_nodes=cap, deleting=leaving, active_resources=active, heads=hs, nodes=ns)
            dec = [S.decode_replacement_head(h) for h in hs]
            fits = [d for d in dec if not d["truncated"]]
            written = max([d["node_off"] + d["n_nodes"] for d in fits if d["n_nodes"]] + [0])
            out["short"] = {"total": total3, "truncated": [d["truncated"] for d in dec], "node_off": [d["node_off"] for d in dec], "n_nodes": [d["n_nodes"] for d in dec],
                            "rows_below_identical": bool((ns[:written] == nodes[:written]).all()), "poison_beyond": bool((ns[cap:] == POISON).all()),
                            "unwritten_intact": bool((ns[written:] == POISON).all())}
        if active:
            kh = S.libs()[1]
            import ctypes
            kh.ksh_snapshot_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
            kh.ksh_snapshot_name.restype = ctypes.c_char_p
            names = []
            for a in range(17):
                s = kh.ksh_snapshot_name(parsed._p, 2, a, 0)
                names.append(None if s is None else s.decode())
            out["resource_names"] = names
        return json.loads(json.dumps(out, default=lambda o: o.tolist() if hasattr(o, "tolist") else list(o)))
    finally:
        parsed.close()


def option_run(S):
    """ksh_replacement_option and the Python mirror's Commands."""
    from karpenter_core_amd import consolidation as C
    out = {}
    snap = _handmade_deleting()      # n2 is deleting
    parsed, pod_node, leaving = C._command_snapshot(snap)
    try:
        TW = 1
        why = [11, 0, 0, 0, 0]      # n0 PDB-blocked
        for tag, cands, wy in (("first_eligible", [0, 2, 3, 1], why), ("nobody", [0, 2], why), ("empty", [], why), ("small_table", [3], [0] * 5)):
            before = S.whatifs_simulated()
            head, nodes, total, pos, ms = S.replacement_option(parsed, pod_node, cands, wy, TW, cap_nodes=8 if tag != "small_table" else 1, deleting=leaving)
            d = S.decode_replacement_head(head)
            d["action"] = ACTIONS[d["action"]]
            out[tag] = {"head": d, "pos": pos, "total": total, "rows": len(nodes), "ms": ms, "row_ids": [[int(r[0]) & 0xFFFFFFFF, int(r[0]) >> 32] for r in nodes],
                        "simulated": S.whatifs_simulated() - before}
        # the counter itself: a batch of four live sets and one that names the deleting node simulates four
        before = S.whatifs_simulated()
        S.replacement_commands(parsed, pod_node, [[3], [0], [2], [1], [4]], TW, cap_nodes=16, deleting=leaving)
        out["batch_of_five_simulated"] = S.whatifs_simulated() - before
        # ksh_replacement_rows over handles the caller keeps open: the same heads and rows as the snapshot call gives for the same sets (flags built by the caller)
        sets = [[3], [0], [4]]
        flats = S.open_whatifs(parsed, pod_node, [list(cs) + list(leaving) for cs in sets], device=0)
        try:
            S.solve_batch_resident(flats)
            hp, npz = np.full((3, S.KS_REP_HEAD_WORDS), POISON, dtype=np.uint64), np.full((9, S.replacement_node_words(TW)), POISON, dtype=np.uint64)
            h1, n1, t1 = S.replacement_rows(flats, [7, 8, 9], [0, S.KS_REP_F_BLOCKED, 0], TW, 9, heads=hp, nodes=npz)
        finally:
            for f in flats:
                f.close()
        h2, n2, t2, _ = S.replacement_commands(parsed, pod_node, sets, TW, cap_nodes=9, deleting=leaving)
        d1, d2 = [S.decode_replacement_head(h) for h in h1], [S.decode_replacement_head(h) for h in h2]
        out["rows"] = {"ids": [d["id"] for d in d1], "blocked": [d["blocked"] for d in d1], "n_nodes": [d["n_nodes"] for d in d1], "node_off": [d["node_off"] for d in d1],
                       "actions": [ACTIONS[d["action"]] for d in d1], "n_new_equal": [a["n_new"] == b["n_new"] and a["n_unscheduled"] == b["n_unscheduled"] for a, b in zip(d1, d2)],
                       "total": t1, "first_rows_equal": bool((n1[:d1[0]["n_nodes"], 1:] == n2[:d2[0]["n_nodes"], 1:]).all()), "beyond_intact": bool((npz[t1:] == POISON).all()),
                       "snapshot_n_nodes": [d["n_nodes"] for d in d2], "last_rows_equal": bool((n1[d1[2]["node_off"]:t1, 1:] == n2[d2[2]["node_off"]:t2, 1:]).all())}
    finally:
        parsed.close()
    # the mirror: "most expired first" (suite_test.go:536) and "one drifted node at a time" (:424 is the flag; :332 the three replacements)
    NOW, S_NS = 1_700_000_000 * 10 ** 9, 10 ** 9
    snap, _, _, _ = TC.replacement_scenarios()["first_candidate_only"]
    info = C.CandidateInfo(node_age_seconds=[0.0, 0.0], now_unix_nanos=NOW, node_creation_unix_nanos=[NOW - 500 * S_NS, NOW - 100 * S_NS], ttl_seconds_until_expired=60, drifted=[1], drift_enabled=True)
    out["expire_most_expired"] = list(C.expiration_command_dev(snap, info).canonical())
    info.node_creation_unix_nanos = [NOW - 100 * S_NS, NOW - 500 * S_NS]
    out["expire_other_order"] = list(C.expiration_command_dev(snap, info).canonical())
    out["drift_one"] = list(C.drift_command_dev(snap, info).canonical())
    info.drift_enabled = False
    out["drift_flag_off"] = list(C.drift_command_dev(snap, info).canonical())
    snap3, _, _, _ = TC.replacement_scenarios()["replace_with_three"]
    cmd = C.drift_command_dev(snap3, C.CandidateInfo(node_age_seconds=[0.0], drifted=[0], drift_enabled=True))
    out["drift_three"] = {"action": cmd.action, "remove": cmd.nodes_to_remove, "replacements": [[list(o), [[k, [v[0], list(v[1]), v[2], v[3]]] for k, v in r]] for o, r in cmd.replacements]}
    un = TDR._uninitialised_neighbour_that_cannot_help()
    out["uninitialised"] = list(C.drift_command_dev(un, C.CandidateInfo(node_age_seconds=[0.0, 0.0], drifted=[0], drift_enabled=True)).canonical())
    return json.loads(json.dumps(out, default=list))


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_replacement_commands as T
out = {}
for name in jobs["names"]:
    try:
        out[name] = T.device_run(S, name)
    except Exception as e:
        import traceback
        out[name] = {"error": repr(e)[:300] + traceback.format_exc()[-1500:]}
print("RESULT " + json.dumps(out))
"""


def run_in_child(names, sim, tmp):
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    path = os.path.join(tmp, "jobs.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "names": names}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in names}
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return run_in_child(CASES + ["option"], True, str(tmp_path_factory.mktemp("replacement_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return run_in_child(CASES + ["option"], bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("replacement_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


def _got(res, name):
    got = res[name]
    assert "error" not in got, got["error"]
    return got


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_heads_and_node_rows_match_the_reference(request, backend, name):
    """Every head (action, why, blocked flag, counts, n_nodes, node_off as the exclusive sum in what-if order, the option popcount) and every node row (options,
    requirements, requests, the id word) of every case; the total; and the sizing call's heads equal the real call's but for the truncated flag."""
    got, want = _got(request.getfixturevalue(backend), name), ref(name)
    off = 0
    for i, (g, w) in enumerate(zip(got["exact"], want)):
        where = (name, i)
        assert (g["id"], g["action"], g["why"], g["blocked"], g["truncated"], g["reserved"]) == (i, w["action"], w["why"], w["blocked"], False, 0), (where, g)
        assert (g["n_new"], g["n_unscheduled"], g["n_nodes"], g["node_off"]) == (w["n_new"], w["n_unscheduled"], len(w["nodes"]), off), (where, g)
        assert g["n_options"] == sum(len(x["options"]) for x in w["nodes"]), where
        assert len(g["nodes"]) == len(w["nodes"])
        for j, (gn, wn) in enumerate(zip(g["nodes"], w["nodes"])):
            assert (gn["id"], gn["node"]) == (i, j), where
            assert gn["options"] == wn["options"] and gn["n_options"] == len(wn["options"]), (where, j)
            assert gn["requirements"] == wn["requirements"], (where, j, gn["requirements"], wn["requirements"])
            assert gn["requests"] == wn["requests"], (where, j, gn["requests"], wn["requests"])
        off += len(w["nodes"])
    assert got["total"] == got["total_exact"] == off
    for s, g in zip(got["sizing"], got["exact"]):
        assert {k: v for k, v in s.items() if k not in ("truncated", "nodes", "action")} == {k: v for k, v in g.items() if k not in ("truncated", "nodes", "action")}
        assert s["truncated"] == (g["n_nodes"] > 0)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_row_hygiene_and_capacity(request, backend, name):
    """Poisoned, wider and longer tables: every word of every row written, surplus and reserved words zero, rows otherwise identical, nothing beyond the rows touched.
    One row short: KS_OK with the full total, complete heads, the truncated flag exactly on the sets that do not fit, identical rows below, the poison beyond intact."""
    got, want = _got(request.getfixturevalue(backend), name), ref(name)
    assert all(got["hygiene"].values()), got["hygiene"]
    if not got["total"]:
        return
    s = got["short"]
    offs = np.cumsum([0] + [len(w["nodes"]) for w in want])
    assert s["total"] == got["total"] and s["node_off"] == [int(x) for x in offs[:-1]] and s["n_nodes"] == [len(w["nodes"]) for w in want]
    assert s["truncated"] == [bool(len(w["nodes"])) and int(offs[i + 1]) > got["total"] - 1 for i, w in enumerate(want)] and any(s["truncated"])
    assert s["rows_below_identical"] and s["poison_beyond"] and s["unwritten_intact"]


def test_the_cases_say_what_they_should():
    """CPU: the reference's own answers on the cases whose point is a particular shape."""
    assert [len(w["nodes"]) for w in ref("rep-replace_with_three")] == [3] and ref("rep-delete_empty")[0]["action"] == "delete" and len(ref("rep-replace_one")[0]["nodes"]) == 1
    h = ref("handmade")
    assert len(h[3]["nodes"]) == 2 and h[4]["n_unscheduled"] > 0 and h[4]["action"] in ("delete", "replace") and h[6]["n_unscheduled"] > 0 and h[6]["action"] == "replace"
    d = ref("deleting_between")
    assert [w["action"] for w in d] == ["replace", "error", "replace", "error", "replace"] and all(len(d[i]["nodes"]) > 0 for i in (0, 2, 4))
    u = ref("uninitialised")[0]
    assert u["action"] == "delete" and u["blocked"] and u["n_new"] >= 1 and CR.replacement_command(case("uninitialised")[0], [0])[0] == "replace"
    b = ref("delete_between")
    assert [len(w["nodes"]) > 0 for w in b] == [True, False, True] and b[1]["action"] == "delete"
    t = ref("t71")[0]
    assert t["nodes"][0]["options"] == [f"t{i:02d}" for i in range(64, 71)] and len(case("t71")[0].instance_types) == 71
    a = ref("active12")[0]
    assert a["action"] == "replace" and "example.com/r5" in a["nodes"][0]["requests"]
    assert len(case("scan")[1]) == SCAN_TILE + 3 and sum(len(w["nodes"]) for w in ref("scan")[:SCAN_TILE]) > 0 and len(ref("scan")[SCAN_TILE]["nodes"]) > 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_active_resource_names(request, backend):
    """Under KSH_ACTIVE_RESOURCES ksh_snapshot_name(what = 2) names the ACTIVE resources (cpu, memory, pods, then the requested one), NULL beyond them."""
    names = _got(request.getfixturevalue(backend), "active12")["resource_names"]
    assert names[:3] == ["cpu", "memory", "pods"] and "example.com/r5" in names and names.count(None) == 17 - 4, names


@pytest.mark.parametrize("backend", BACKENDS)
def test_replacement_option(request, backend):
    """The first candidate with why == 0 that is not deleting decides and ONLY it is simulated; PDB-blocked and deleting candidates are passed over; nobody eligible
    gives an all-zero head; a table too small is answered with the total.  The mirror's Commands equal the reference's."""
    got = _got(request.getfixturevalue(backend), "option")
    snap = _handmade_deleting()
    f = got["first_eligible"]
    w = ref_set(snap, [3])
    assert f["pos"] == 2 and f["head"]["id"] == 2 and f["head"]["action"] == w["action"] == "replace" and f["head"]["n_nodes"] == len(w["nodes"]) == f["total"] == f["rows"]
    assert f["row_ids"] == [[0, j] for j in range(f["total"])]
    for tag in ("nobody", "empty"):
        z = got[tag]
        assert z["pos"] == -1 and z["total"] == 0 and z["head"] == dict(z["head"], id=0, action="do-nothing", why=0, n_new=0, n_nodes=0, node_off=0, n_options=0) and all(v == 0.0 for v in z["ms"].values())
    assert got["small_table"]["total"] == len(w["nodes"]) > 1 and got["small_table"]["rows"] == got["small_table"]["total"]      # (cap_nodes 1 was too small: called again)
    # exactly ONE what-if is opened and solved, however many candidates are listed (ksh_whatifs_simulated counts them behind the ABI); none when nobody is eligible;
    # the wrapper's second call with a larger table is a second simulation of that one set; a batch simulates its live sets, not the one naming a deleting node
    assert f["simulated"] == 1 and got["nobody"]["simulated"] == 0 and got["empty"]["simulated"] == 0 and got["small_table"]["simulated"] == 2
    assert got["batch_of_five_simulated"] == 4
    assert f["ms"]["open_ms"] > 0.0 and f["ms"]["solve_ms"] > 0.0
    # the Commands
    s2, _, _, _ = TC.replacement_scenarios()["first_candidate_only"]
    assert got["expire_most_expired"] == list(_canon(D.replacement_command(s2, [0, 1], TDR.simulate)))
    assert got["expire_other_order"] == list(_canon(D.replacement_command(s2, [1, 0], TDR.simulate)))
    assert got["expire_most_expired"][1] == ["to-expire"] and got["expire_other_order"][1] == ["not-yet"]
    assert got["drift_one"] == list(_canon(D.replacement_command(s2, [1], TDR.simulate))) and got["drift_flag_off"] == ["do-nothing", [], [], []]
    s3, _, _, _ = TC.replacement_scenarios()["replace_with_three"]
    lit = D.replacement_command(s3, [0], TDR.simulate)
    assert got["drift_three"]["action"] == "replace" and got["drift_three"]["remove"] == lit[1] and len(got["drift_three"]["replacements"]) == len(lit[2]) == 3
    for (opts, reqs), n in zip(got["drift_three"]["replacements"], lit[2]):
        assert opts == list(n.instance_types) and dict((k, v) for k, v in reqs) == _reqs(n)
    assert got["uninitialised"][0] == "delete" and got["uninitialised"][1] == ["n1"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_replacement_rows_over_open_handles(request, backend):
    """ksh_replacement_rows for a caller that keeps its what-ifs open: its own ids, its own flags (the second set flagged blocked: a delete without rows), the same counts,
    offsets and node rows (but for the id word) as the snapshot call over the same sets; nothing written beyond the rows."""
    r = _got(request.getfixturevalue(backend), "option")["rows"]
    assert r["ids"] == [7, 8, 9] and r["blocked"] == [False, True, False] and r["actions"] == ["replace", "delete", "replace"] and all(r["n_new_equal"])
    assert r["n_nodes"] == [r["snapshot_n_nodes"][0], 0, r["snapshot_n_nodes"][2]] and r["snapshot_n_nodes"][1] > 0
    assert r["node_off"] == [0, r["n_nodes"][0], r["n_nodes"][0]] and r["total"] == r["n_nodes"][0] + r["n_nodes"][2]
    assert r["first_rows_equal"] and r["last_rows_equal"] and r["beyond_intact"]


def _canon(cmd):
    action, remove, new_nodes, _ = cmd
    first = new_nodes[0] if new_nodes else None
    return (action, list(remove), list(first.instance_types) if first else [], [[k, v] for k, v in sorted(_reqs(first).items())] if first else [])


def test_the_layout_constants_are_the_headers():
    import re
    from karpenter_core_amd import scheduler as S
    hdr = open(os.path.join(ROOT, "include", "ksolve.h")).read()
    for name in ("KS_REP_HEAD_WORDS", "KS_REP_ID", "KS_REP_DECISION", "KS_REP_N_NEW", "KS_REP_N_UNSCHEDULED", "KS_REP_N_NODES", "KS_REP_NODE_OFF", "KS_REP_N_OPTIONS", "KS_REP_NODE_ID",
                 "KS_REP_NODE_PRESENT", "KS_REP_NODE_IT_STATE", "KS_REP_NODE_N_OPTIONS", "KS_REP_NODE_REQMASK", "KS_REP_NODE_MASK", "KS_REP_NODE_BOUNDS", "KS_REP_NODE_REQ", "KS_REP_NODE_OPTIONS",
                 "KS_REP_BLOCKED", "KS_REP_TRUNCATED", "KS_REP_F_BLOCKED", "KS_MAX_RES"):
        m = re.search(r"#define %s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(S, name), name
    assert S.KS_REP_NODE_BOUNDS - S.KS_REP_NODE_MASK == 32 and S.KS_REP_NODE_REQ - S.KS_REP_NODE_BOUNDS == 32 and S.KS_REP_NODE_OPTIONS - S.KS_REP_NODE_REQ == S.KS_MAX_RES
