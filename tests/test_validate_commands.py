"""Consolidation commands validated on the device (include/kshost.h ksh_validate_commands / ksh_single_node_resume / ksh_validate_empty_nodes; kernel
ks_validate_commands in csrc/ksolve.hip) against the literal restatement oracle/consolidation_ref.py::validate_command, one oracle Solve per command.

A case is the cluster as it is NOW -- a snapshot of tests/test_consolidation.py / tests/test_consolidation_commands.py (imported, not copied) with a small change --,
what candidate selection reads beside it, and a few commands computed (or written down) a TTL earlier.  Every case runs twice, in the shape of
tests/test_consolidation_commands.py: unmarked on the emulator build of the kernels in a child process, and marked `gpu` on the device.  `device_run` is the part that
needs the kernels; every comparison happens here."""
import copy
import dataclasses
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import consolidation as C, fake
from karpenter_core_amd.model import LABEL_CAPACITY_TYPE as CT, LABEL_INSTANCE_TYPE, LABEL_PROVISIONER, LABEL_ZONE as ZONE, Offering
from oracle import consolidation_ref as CR

import test_consolidation as TC
import test_consolidation_commands as TCC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POISON = 0xA5A5A5A5DEADBEEF
INVALID, VALID, ERROR = 0, 1, 2
WHY_VALID, WHY_NOMINATED, WHY_NO_CANDIDATES, WHY_DELETING, WHY_NOT_ALL_SCHEDULED, WHY_NO_NEW_NODE, WHY_MANY_NODES, WHY_UNEXPECTED_NODE, WHY_NOT_A_SUBSET = range(9)
F_BLOCKED, F_EXPECT_REPLACEMENT = 1, 2


# ---------------------------------------------------------------------------------------------------------------- the cases
def info(n, **kw):
    return C.CandidateInfo(node_age_seconds=[0.0] * n, **kw)


def _then_commands():
    """tests/test_consolidation_commands.py's handmade cluster a TTL ago (nodes: 0 n-spot, 1 n-od, 2 n-od-pin, 3 n-two, 4 n-huge, all full) and the two replaces
    computeConsolidation finds there."""
    then = TCC._handmade()
    od, pin = CR.compute_consolidation(then, [1]), CR.compute_consolidation(then, [2])
    assert od[0] == pin[0] == "replace" and "spot-cheap" in od[2]
    return ("replace", ["n-od"], list(od[2])), ("replace", ["n-od-pin"], list(pin[2]))


def _wide_catalogue(lost):
    """T = 71 > 64: seventy cheap types and `big`, one full node on `big`; NOW type `lost` has no available offering any more."""
    its = [fake.new_instance_type(f"t{i:02d}", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("on-demand", "z-a", 0.1 + 0.001 * i, True)]) for i in range(70)]
    its.append(fake.new_instance_type("big", {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering("on-demand", "z-a", 2.0, True)]))
    n = TC.node("n0", its[70], "on-demand", "z-a", cpu="4")
    n.available = {"cpu": "0", "pods": "10"}
    then = TC.snapshot(its, [n], [[TC.pod("p0")]])
    cmd = CR.compute_consolidation(then, [0])
    assert cmd[0] == "replace" and len(cmd[2]) == 70
    now = copy.deepcopy(then)
    now.instance_types[lost].offerings = [Offering("on-demand", "z-a", 0.1, False)]
    return now, ("replace", ["n0"], list(cmd[2]))


_BUILT = {}


def case(name):
    """-> {"now": Snapshot, "info": CandidateInfo, "late": nodes marked for deletion after the candidates were listed, "commands": [(action, node names, type names)]}"""
    if name in _BUILT:
        return _BUILT[name]
    od, pin = _then_commands()
    now, late, inf, cmds = TCC._handmade(), [], None, [od, pin]
    if name == "unchanged":          # two valid replaces; a hand-written replace of the node whose two pods exclude each other's zones (6); the node whose pod fits nothing (4)
        cmds = [od, ("replace", ["n-two"], ["both"]), pin, ("replace", ["n-huge"], ["both"]), ("delete", ["n-od"], [])]      # the last: a delete that needs a node (7)
    elif name == "unchanged_delete":
        now, cands, _ = TC.scenarios()["can_delete_nodes"]
        cmds = [("delete", ["n1"], []), ("replace", ["n1"], [now.instance_types[0].name])]      # the second: a replace whose pods fit the rest (5)
    elif name == "nominated":
        inf = info(5, nominated=[1])
        cmds = [od, pin, ("replace", ["n-od-pin", "n-od"], list(pin[2])), pin]
    elif name == "do_not_consolidate":
        inf = info(5, do_not_consolidate={1: "true", 2: "false"})      # ("false": passes without the provisioner checks)
        cmds = [od, pin, ("replace", [], list(pin[2])), ("delete", ["no-such-node"], [])]
    elif name == "consolidation_disabled":
        inf = info(5, consolidation_enabled=False)
    elif name == "late_deleting":
        late = [1]
        cmds = [pin, od, pin]
    elif name == "pod_fits_nowhere":
        now.bound[1].append(TC.pod("p-late", "64"))
    elif name == "uninitialised_neighbour":
        del now.nodes[0].labels["karpenter.sh/initialized"]
    elif name == "fits_the_rest":
        now.nodes[0].available = {"cpu": "4", "pods": "10"}
    elif name == "delete_needs_a_node":
        now, _, _ = TC.scenarios()["can_delete_nodes"]
        now.bound[1].extend(TC.pod(f"late-{i}", "6") for i in range(5))
        now.nodes[1].available = dict(now.nodes[1].available, cpu="1")
        now.bound[0][0] = TC.pod("p1", "2")
        cmds = [("delete", ["n1"], [])]
    elif name == "lost_offering":
        now.instance_types[0].offerings = [Offering("spot", "z-a", 0.1, False), Offering("spot", "z-b", 0.15, False)]
    elif name == "wide_high":
        now, cmd = _wide_catalogue(66)
        cmds = [cmd]
    elif name == "wide_low":
        now, cmd = _wide_catalogue(5)
        cmds = [cmd]
    else:
        raise KeyError(name)
    out = {"now": now, "info": inf or info(len(now.nodes)), "late": late, "commands": cmds}
    _BUILT[name] = out
    return out


CASES = ["unchanged", "unchanged_delete", "nominated", "do_not_consolidate", "consolidation_disabled", "late_deleting", "pod_fits_nowhere", "uninitialised_neighbour",
         "fits_the_rest", "delete_needs_a_node", "lost_offering", "wide_high", "wide_low"]


def events_case():
    """The events route.  THEN is the handmade cluster; NODE- n-spot, UNBIND p-od, BIND p-od2 (which insists on on-demand) to n-od; n-two is annotated do-not-consolidate.
    -> (then, events, the freshly ingested equivalent NOW, its info, the info over THEN's slots, commands)"""
    od, pin = _then_commands()
    then = TCC._handmade()
    p2 = TC.pod("p-od2")
    p2.node_selector = {CT: "on-demand"}
    events = [("node-", "n-spot"), ("unbind", "p-od"), ("bind", "n-od", p2)]
    fresh = TCC._handmade()
    fresh.nodes, fresh.bound = fresh.nodes[1:], [[copy.deepcopy(p2)]] + fresh.bound[2:]
    cmds = [("replace", ["n-spot", "n-two", "n-od-pin"], list(pin[2])),      # partial mapping: one node left, one is no candidate any more, the third is simulated
            ("replace", ["n-spot", "n-od"], list(od[2])), ("delete", ["n-spot"], []), pin]
    return then, events, fresh, info(4, do_not_consolidate={2: "true"}), info(5, do_not_consolidate={3: "true"}), cmds


# ---------------------------------------------------------------------------------------------------------------- the reference
def ref_candidates(snap, inf, deleting=()):
    """candidateNodes (helpers.go:171-230) with consolidation.ShouldDeprovision (consolidation.go:106-121) as its filter, literally: the node indices mapNodes maps onto."""
    prov_types = {snap.instance_types[t].name for t in snap.provisioner.instance_types}
    out = []
    for i, n in enumerate(snap.nodes):
        lab = n.labels
        if not n.in_state or i in deleting or lab.get(LABEL_PROVISIONER) != snap.provisioner.name or lab.get(LABEL_INSTANCE_TYPE) not in prov_types:
            continue
        if CT not in lab or ZONE not in lab or lab.get("karpenter.sh/initialized") != "true" or i in inf.nominated:
            continue
        if i in inf.do_not_consolidate:
            if inf.do_not_consolidate[i] == "true":
                continue
        elif not inf.consolidation_enabled:
            continue
        out.append(i)
    return out


def ref_row(now, inf, late, cmd):
    """Validation.IsValid after its wait: the nomination check, then CR.validate_command; the step that decided is read off the same simulation with CR's predicates."""
    action, names, types = cmd
    slot = {n.name: j for j, n in enumerate(now.nodes)}
    idxs = [slot[n] for n in names if n in slot]
    if any(j in inf.nominated for j in idxs):
        return {"valid": False, "why": WHY_NOMINATED, "n_mapped": 0}
    cands = ref_candidates(now, inf, now.deleting)
    snap = dataclasses.replace(now, deleting=tuple(now.deleting) + tuple(late))
    mapped = sorted({j for j in idxs if j in cands})
    try:
        valid = CR.validate_command(snap, action, names, types, cands)
    except ValueError:
        return {"valid": None, "why": WHY_DELETING, "n_mapped": len(mapped)}
    if not mapped:
        assert valid is False
        return {"valid": False, "why": WHY_NO_CANDIDATES, "n_mapped": 0}
    sink = []
    CR.compute_consolidation(snap, mapped, sink)
    res = sink[0]
    gone = set(mapped) | set(snap.deleting)
    blocked = any(n.in_state and n.owned and n.labels.get("karpenter.sh/initialized") != "true" for j, n in enumerate(snap.nodes) if j not in gone)
    now_types = list(res.new_nodes[0].instance_types) if res.new_nodes else []
    missing = []
    if blocked or res.unscheduled:
        why = WHY_NOT_ALL_SCHEDULED
    elif not res.new_nodes:
        why = WHY_NO_NEW_NODE if types else WHY_VALID
    elif len(res.new_nodes) > 1:
        why = WHY_MANY_NODES
    elif not types:
        why = WHY_UNEXPECTED_NODE
    else:
        missing = sorted(set(types) - set(now_types))
        why = WHY_NOT_A_SUBSET if missing else WHY_VALID
    assert valid == (why == WHY_VALID)
    return {"valid": valid, "why": why, "n_mapped": len(mapped), "n_new": len(res.new_nodes), "n_unscheduled": len(res.unscheduled), "options": sorted(now_types), "missing": missing,
            "blocked": blocked}


_REF = {}


def ref_case(name):
    if name not in _REF:
        c = case(name)
        _REF[name] = [ref_row(c["now"], c["info"], c["late"], cmd) for cmd in c["commands"]]
    return _REF[name]


# ---------------------------------------------------------------------------------------------------------------- the device side
def _named(snap, d):
    d = dict(d)
    d["options"], d["missing"] = sorted(snap.instance_types[t].name for t in d["options"]), sorted(snap.instance_types[t].name for t in d["missing"])
    return d


def _validate(S, snap, parsed, pod_node, leaving, why, nf, cmds, late, words=None, out=None):
    tw = (len(snap.instance_types) + 63) // 64
    node_sets, expect, type_sets = C._command_inputs_now(snap, [C.Command(a, list(n), list(t)) for a, n, t in cmds])
    rows, _ = S.validate_commands(parsed, pod_node, node_sets, expect, type_sets, why, nf, words or tw, deleting=list(leaving) + list(late), out=out)
    return rows


def device_run(S, name):
    """One case on one backend: the decoded rows of ksh_validate_commands, and the same call into a poisoned buffer with rows two words wider than the catalogue needs."""
    c = case(name)
    now, cmds = c["now"], c["commands"]
    tw = (len(now.instance_types) + 63) // 64
    parsed, pod_node, leaving = C._command_snapshot(now)
    try:
        got, nf = C._candidates_call(S, parsed, pod_node, now, c["info"])
        rows = _validate(S, now, parsed, pod_node, leaving, got["why"], nf, cmds, c["late"])
        out = {"rows": [_named(now, S.decode_validation_row(r, tw)) for r in rows], "why_of_nodes": [int(x) for x in got["why"]]}
        wide = tw + 2
        buf = np.full((len(cmds), S.validation_row_words(wide)), POISON, dtype=np.uint64)
        wrows = _validate(S, now, parsed, pod_node, leaving, got["why"], nf, cmds, c["late"], words=wide, out=buf)
        out["hygiene"] = {"poison_left": int((wrows == np.uint64(POISON)).sum()), "reserved_zero": bool((wrows[:, 7] == 0).all()),
                          "tails_zero": bool((wrows[:, 8 + tw:8 + wide] == 0).all() and (wrows[:, 8 + wide + tw:] == 0).all()),
                          "same": all(np.array_equal(np.concatenate([wrows[i, :8 + tw], wrows[i, 8 + wide:8 + wide + tw]]), rows[i]) for i in range(len(cmds)))}
        if name == "unchanged":       # the Python mirror, names in, verdicts out
            out["mirror"] = [[v, w] for v, w in C.validate_commands_dev(now, [C.Command(a, list(n), list(t)) for a, n, t in cmds], c["info"])]
        return out
    finally:
        parsed.close()


def events_run(S):
    """NOW reached by ksh_env_apply on the parsed THEN snapshot (pod_node = NULL afterwards) against a freshly ingested equivalent; rows by NAME."""
    then, events, fresh, finfo, tinfo, cmds = events_case()
    tw = (len(then.instance_types) + 63) // 64
    out = {}
    parsed, pod_node, leaving = C._command_snapshot(then)
    try:
        parsed.apply(events, pod_node)
        bind, n_nodes = parsed.bindings()
        nf = [0] * n_nodes
        for i, v in tinfo.do_not_consolidate.items():
            nf[i] |= S.KSH_CAND_NODE_DO_NOT_CONSOLIDATE | (S.KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE if v == "true" else 0)
        got = S.consolidation_candidates(parsed, None, nf, [0.0] * n_nodes, [0] * len(bind), [0.0] * len(bind), [0] * len(bind), [True], [None])
        rows = _validate(S, then, parsed, None, leaving, got["why"], nf, cmds, [])      # (names -> slots of THEN: slots are stable across events)
        out["events"] = [_named(then, S.decode_validation_row(r, tw)) for r in rows]
        out["why_of_nodes"] = [int(x) for x in got["why"]]
    finally:
        parsed.close()
    parsed, pod_node, leaving = C._command_snapshot(fresh)
    try:
        got, nf = C._candidates_call(S, parsed, pod_node, fresh, finfo)
        rows = _validate(S, fresh, parsed, pod_node, leaving, got["why"], nf, cmds, [])
        out["fresh"] = [_named(fresh, S.decode_validation_row(r, tw)) for r in rows]
    finally:
        parsed.close()
    return out


def _raw_call(S, parsed, pod_node, words, n=1, off=(0, 1), nodes=(1,), expect=(0,), why=(0,) * 5, nf=(0,) * 5, flags=0, options=None, null=None, rows=None):
    import ctypes
    kh = S.libs()[1]
    arr = {"off": S._u32s(off), "nodes": S._u32s(nodes), "expect": S._u32s(expect), "why": S._u32s(why), "nf": S._u32s(nf),
           "options": np.zeros((n, max(1, words)), dtype=np.uint64) if options is None else np.ascontiguousarray(np.asarray(options, dtype=np.uint64))}
    ptr = {k: (None if k == null else v.ctypes.data) for k, v in arr.items()}
    pn = np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32))
    kh.ksh_validate_commands.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 8 + [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    rc = kh.ksh_validate_commands(parsed._p, flags, n, ptr["off"], ptr["nodes"], ptr["expect"], ptr["options"], ptr["why"], ptr["nf"], pn.ctypes.data, None, 0, 0,
                                  None if null == "rows" else rows.ctypes.data, words, None)
    return [rc, kh.ksh_last_error().decode() if rc != S.KS_OK else ""]


def refusals_run(S):
    """Every whole-call refusal's return code and message, into poisoned rows; then the same snapshot still answers."""
    now = TCC._handmade()
    T = len(now.instance_types)
    tw = (T + 63) // 64
    parsed, pod_node, _ = C._command_snapshot(now)
    out = {}
    try:
        rows = np.full((2, S.validation_row_words(tw)), POISON, dtype=np.uint64)
        call = lambda **kw: _raw_call(S, parsed, pod_node, kw.pop("words", tw), rows=rows, **kw)
        out["flag_bit"] = call(flags=1 << 20)
        out["words_short"] = call(words=tw - 1)
        out["offsets"] = call(n=2, off=(0, 1, 0), nodes=(1, 1), expect=(0, 0))
        out["slot"] = call(nodes=(5,))
        out["type_index"] = call(expect=(1,), options=[[1 << T]])
        for k in ("off", "expect", "why", "nf", "rows"):
            out["null_" + k] = call(null=k)
        out["null_options"] = call(expect=(1,), null="options")
        out["untouched"] = bool((rows == np.uint64(POISON)).all())
        out["then_answers"] = call()
        out["answer"] = S.decode_validation_row(rows[0], tw)
    finally:
        parsed.close()
    return out


def replays_run(S):
    """ksh_single_node_resume over the handmade cluster, and ksh_validate_empty_nodes over arrays written down here."""
    out = {"resume": {}, "empty": []}
    for tag, (cands, failed_before, kw) in RESUME.items():
        now = TCC._handmade()
        state, cmd = C.single_node_resume_dev(now, cands, failed_before, info(5, **kw))
        out["resume"][tag] = [state, list(cmd.canonical())]
    for nodes, why, n_pods, nf in EMPTY:
        out["empty"].append(S.validate_empty_nodes(nodes, why, n_pods, nf))
    now = TCC._handmade()
    now.nodes.append(TC.node("n-empty", now.instance_types[3], "on-demand", "z-a"))
    now.bound.append([])
    out["empty_mirror"] = [C.validate_empty_nodes(now, ["n-empty"], info(6)), C.validate_empty_nodes(now, ["n-empty", "n-od"], info(6)), C.validate_empty_nodes(now, ["n-od"], info(6, nominated=[1]))]
    return out


# candidate order, failedValidation so far, what candidate selection reads: n-huge and n-spot give do-nothing, n-od and n-od-pin a replace
RESUME = {"found": ([4, 0, 1, 2], False, {}), "found_after_failure": ([4, 1, 2], False, {"do_not_consolidate": {1: "true"}}), "retry_failed_before": ([4, 0], True, {}),
          "do_nothing": ([4, 0], False, {}), "retry_failure_inside": ([4, 1], False, {"do_not_consolidate": {1: "true"}}), "retry_nominated": ([1], False, {"nominated": [1]}),
          "none_left": ([], False, {})}
# (the command's nodes, why / bound pods / flags per node slot)
EMPTY = [([0, 1], [0, 0, 0], [0, 0, 3], [0, 0, 0]), ([0, 1], [0, 0, 0], [0, 2, 0], [0, 0, 0]), ([0, 1], [0, 0, 0], [0, 2, 0], [0, 1, 0]), ([1], [0, 9, 0], [0, 2, 0], [0, 0, 0]),
         ([1, 2], [0, 13, 7], [0, 2, 2], [0, 0, 0]), ([2], [0, 0, 11], [0, 0, 1], [0, 0, 0]), ([], [0], [1], [0])]


def ref_resume(now, cands, failed_before, inf):
    """singlenodeconsolidation.go:54-84 from a candidate on, literally, over CR.compute_consolidation and CR.validate_command."""
    failed = failed_before
    still = ref_candidates(now, inf, now.deleting)
    for c in cands:
        try:
            cmd = CR.compute_consolidation(now, [c])
        except ValueError:
            continue
        if cmd[0] == "do-nothing":
            continue
        try:
            valid = c not in inf.nominated and CR.validate_command(now, cmd[0], cmd[1], cmd[2], still)
        except ValueError:
            continue
        if not valid:
            failed = True
            continue
        return ["found", json.loads(json.dumps(list(CR.canonical(cmd))))]
    return ["retry" if failed else "do-nothing", json.loads(json.dumps(list(C.Command().canonical())))]


def ref_empty(nodes, why, n_pods, nf):
    """emptynodeconsolidation.go:77-87, literally: mapNodes, then `len(n.pods) != 0 && !IsNodeNominated` -> retry.  Nothing mapped: the loop does not run, the command stands."""
    mapped = [c for c in range(len(why)) if why[c] in (0, 10, 11, 12) and c in nodes]
    for n in mapped:
        if n_pods[n] != 0 and not (nf[n] & 1):
            return True
    return False


SPECIAL = {"events": events_run, "refusals": refusals_run, "replays": replays_run}

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_validate_commands as T
out = {}
for name in jobs["names"]:
    try:
        out[name] = T.SPECIAL[name](S) if name in T.SPECIAL else T.device_run(S, name)
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
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in names}
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return run_in_child(CASES + list(SPECIAL), True, str(tmp_path_factory.mktemp("validate_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return run_in_child(CASES + list(SPECIAL), bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("validate_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


def _got(res, name):
    got = res[name]
    assert "error" not in got, got["error"]
    return got


def _same_row(row, want, where):
    assert (row["valid"], row["why"], row["n_mapped"], row["reserved"]) == (want["valid"], want["why"], want["n_mapped"], 0), (where, row, want)
    if want["why"] in (WHY_NOMINATED, WHY_NO_CANDIDATES, WHY_DELETING):      # written by the library, never simulated
        assert (row["n_new"], row["n_unscheduled"], row["n_options"], row["n_missing"], row["options"], row["missing"]) == (0, 0, 0, 0, [], []), (where, row)
        return
    assert (row["n_new"], row["n_unscheduled"]) == (want["n_new"], want["n_unscheduled"]), (where, row, want)
    assert row["options"] == want["options"] and row["n_options"] == len(want["options"]), (where, row, want)
    assert row["missing"] == want["missing"] and row["n_missing"] == len(want["missing"]), (where, row, want)


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_rows_match_validate_command(request, backend, name):
    """Every command of every case: verdict, the step that decided, the counts, the re-simulation's options and the command's missing types, against the oracle.  Row i
    answers command i, also where rows the library writes (1-3) sit between simulated ones."""
    got = _got(request.getfixturevalue(backend), name)
    want = ref_case(name)
    assert len(got["rows"]) == len(want)
    for i, (row, w) in enumerate(zip(got["rows"], want)):
        assert row["id"] == i
        _same_row(row, w, (name, i))
    if "mirror" in got:
        assert got["mirror"] == [[w["valid"], w["why"]] for w in want]


def test_every_why_is_reached_by_the_cases():
    """(CPU, the oracle alone) Over the committed cases every code 0-8 occurs; 4 both ways (a pod that fits nowhere, an uninitialised node that stays); 0 for a delete and
    for a replace; rows of the library between simulated rows in one call."""
    whys, valid_actions, four = set(), set(), set()
    for name in CASES:
        for cmd, w in zip(case(name)["commands"], ref_case(name)):
            whys.add(w["why"])
            if w["why"] == WHY_VALID:
                valid_actions.add(cmd[0])
            if w["why"] == WHY_NOT_ALL_SCHEDULED:
                four.add("blocked" if w["blocked"] and not w["n_unscheduled"] else "unscheduled")
    assert whys == set(range(9)), whys
    assert valid_actions == {"delete", "replace"} and four == {"blocked", "unscheduled"}
    for name in ("nominated", "do_not_consolidate", "late_deleting"):
        w = [r["why"] in (1, 2, 3) for r in ref_case(name)]
        assert any(a and not b for a, b in zip(w, w[1:])) and any(b and not a for a, b in zip(w, w[1:])), name


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_subset_test_crosses_a_word_boundary(request, backend):
    """T = 71: the one type the command lists and the re-simulation lacks has index 66 (second word) in one case and 5 in the other; KS_VAL_N_MISSING and the second
    option block name exactly that type."""
    res = request.getfixturevalue(backend)
    for name, lost in (("wide_high", 66), ("wide_low", 5)):
        now = case(name)["now"]
        assert len(now.instance_types) == 71
        row = _got(res, name)["rows"][0]
        assert (row["valid"], row["why"], row["n_missing"], row["missing"]) == (False, WHY_NOT_A_SUBSET, 1, [now.instance_types[lost].name]), row
        assert row["n_options"] == 70 and now.instance_types[lost].name not in row["options"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_events_route_and_partial_mapping(request, backend):
    """NOW reached by ksh_env_apply (NODE-, UNBIND, BIND) with pod_node = NULL: the rows equal those over a freshly ingested equivalent snapshot, by name, and both equal
    the reference.  Command 0 names three nodes of which one left and one is no candidate any more: only the third is simulated."""
    got = _got(request.getfixturevalue(backend), "events")
    then, events, fresh, finfo, tinfo, cmds = events_case()
    assert got["why_of_nodes"] == [13, 0, 0, 8, 0]
    assert got["events"] == got["fresh"]
    want = [ref_row(fresh, finfo, [], cmd) for cmd in cmds]
    for i, (row, w) in enumerate(zip(got["events"], want)):
        _same_row(row, w, ("events", i))
    assert got["events"][0]["n_mapped"] == 1 and want[0]["n_mapped"] == 1 and got["events"][0]["valid"] is True
    assert [r["why"] for r in got["events"]] == [WHY_VALID, WHY_NOT_A_SUBSET, WHY_NO_CANDIDATES, WHY_VALID]
    assert got["events"][1]["missing"] == ["spot-cheap"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", CASES)
def test_row_hygiene(request, backend, name):
    """Rows prefilled with a poison word and two words wider than ceil(T/64): every word is written, the surplus words and the reserved word are zero, and the rows are
    those of the narrow call."""
    h = _got(request.getfixturevalue(backend), name)["hygiene"]
    assert h == {"poison_left": 0, "reserved_zero": True, "tails_zero": True, "same": True}


@pytest.mark.parametrize("backend", BACKENDS)
def test_refusals_leave_the_rows_untouched(request, backend):
    got = _got(request.getfixturevalue(backend), "refusals")
    for tag, needle in (("flag_bit", "flag bit"), ("words_short", "too short"), ("offsets", "ascending"), ("slot", "out of range"), ("type_index", "type index"),
                        ("null_off", "null"), ("null_expect", "null"), ("null_why", "null"), ("null_nf", "null"), ("null_rows", "null"), ("null_options", "null")):
        assert got[tag][0] == -1 and needle in got[tag][1], (tag, got[tag])
    assert got["untouched"]
    assert got["then_answers"] == [0, ""] and (got["answer"]["valid"], got["answer"]["why"], got["answer"]["n_new"]) == (False, WHY_UNEXPECTED_NODE, 1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_single_node_resume_replays_the_loop(request, backend):
    got = _got(request.getfixturevalue(backend), "replays")["resume"]
    states = set()
    for tag, (cands, failed_before, kw) in RESUME.items():
        want = ref_resume(TCC._handmade(), cands, failed_before, info(5, **kw))
        assert json.loads(json.dumps(got[tag])) == want, (tag, got[tag], want)
        states.add((want[0], failed_before))
    assert states == {("found", False), ("retry", True), ("retry", False), ("do-nothing", False)}
    assert got["found"][1][1] == ["n-od"] and got["found_after_failure"][1][1] == ["n-od-pin"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_validate_empty_nodes_is_the_reference_loop(request, backend):
    got = _got(request.getfixturevalue(backend), "replays")
    want = [ref_empty(*e) for e in EMPTY]
    assert got["empty"] == want and set(want) == {True, False}
    assert want[3] is False and want[4] is False      # nothing maps: the command is returned as it is
    assert got["empty_mirror"] == [False, True, False]      # an empty node alone; with a node that has a pod; that node nominated (no candidate: it does not map)


def test_the_row_layout_constants_are_the_headers():
    """scheduler.KS_VAL_* and this file's own copies against the #defines of include/ksolve.h."""
    from karpenter_core_amd import scheduler as S
    text = open(os.path.join(ROOT, "include", "ksolve.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (KS_VAL_[A-Z_]+) (\d+)u?\b", text)}
    assert len(defs) >= 22
    for name, value in defs.items():
        if name != "KS_VAL_F_ALL":
            assert getattr(S, name) == value, name
    assert (INVALID, VALID, ERROR) == (defs["KS_VAL_INVALID"], defs["KS_VAL_VALID"], defs["KS_VAL_ERROR"])
    assert tuple(range(9)) == tuple(defs["KS_VAL_WHY_" + n] for n in ("VALID", "NOMINATED", "NO_CANDIDATES", "DELETING", "NOT_ALL_SCHEDULED", "NO_NEW_NODE", "MANY_NODES",
                                                                     "UNEXPECTED_NODE", "NOT_A_SUBSET"))
    assert (F_BLOCKED, F_EXPECT_REPLACEMENT) == (defs["KS_VAL_F_BLOCKED"], defs["KS_VAL_F_EXPECT_REPLACEMENT"])
    assert S.validation_row_words(3) == defs["KS_VAL_OPTIONS"] + 6 == 14


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_validation")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_validation.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    from karpenter_core_amd import workloads as W
    from karpenter_core_amd.model import delta_to_ksd
    then, events, fresh, finfo, _, _ = events_case()
    pr, pod_node = W.snapshot_problem(then.instance_types, then.provisioner, then.nodes, then.bound)
    f, d = tmp_path / "snapshot.ksp", tmp_path / "events.ksd"
    f.write_text(pr.to_ksp())
    d.write_text(delta_to_ksd(events))
    out = subprocess.run([exe, str(f), str(d)] + [str(int(x)) for x in pod_node], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    # THEN: n-od and n-od-pin are replaced; NOW (no annotations in this program): n-od's pod insists on on-demand, n-od-pin is as it was
    od, pin = _then_commands()
    want = [ref_row(fresh, info(4), [], cmd) for cmd in (od, pin)]
    assert [w["why"] for w in want] == [WHY_NOT_A_SUBSET, WHY_VALID]
    assert "validated n-od: invalid (step 8) missing 1: spot-cheap" in out.stdout, out.stdout
    assert "validated n-od-pin: valid" in out.stdout, out.stdout
    assert "refused: validation row too short" in out.stdout, out.stdout


def test_c_abi_from_c_on_the_emulator(tmp_path):
    """tests/cabi_usage_validation.c -- commands at t0, events, candidates and validation at t0 + TTL -- as C99 with -Wall -Werror -pedantic, on the emulator build."""
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_c_abi_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
