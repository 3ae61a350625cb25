"""(CPU) The audit's second pass -- pod (anti-)affinity and hostname spread in commit order (include/ksolve.h ks_audit_topology_dev) -- validated where a correct
result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_topo_ref.py) over every result the lane-fibre emulator returns for its committed cases -- the set
     tests/test_audit.py audits, results proven equal to the oracle's in tests/test_rr_emulated.py -- raises NO flag; a rule that flagged one of them would be a wrong
     rule, not a finding.  The kernels' own source (karpenter_core_amd/csrc/ks_audit_topo.inc) is compiled into the emulator build and runs beside the reference:
     the two agree bit for bit, `checked` included;
  b) the commit-order gate: the rules across nodes rest on pod_seq being the reference's commit order ACROSS nodes.  For problems without existing nodes the oracle's
     KO_TRACE file has one line per Scheduler.add that reached the new nodes; a placed pod's last line is its successful add.  The pods' order by pod_seq must be
     the order of those lines, for ks_pack_rr and for ks_pack;
  c) the tamper matrix and the kernels' other paths (tests/audit_topo_cases.py) on the emulator;
  d) unit cases of the reference alone on a hand-made problem: one per bit and per direction.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import audit_harness as H
import audit_ref as A
import audit_topo_cases as TC
import audit_topo_ref as TR
import test_rr_emulated as E

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
import audit_harness as H, audit_topo_ref as TR, audit_topo_cases as TC
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR
out = {}
def bits(flags):
    return {k: int(((flags & v) != 0).sum()) for k, v in TR.BITS.items() if ((flags & v) != 0).any()}
def audited(name, f):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev = f.audit_topology()
        prob = TR.problem_arrays(S, f)
        seq = H.commit_numbers(S, f, prob)
        flags, checked, skipped = TR.audit(prob, f.result_arrays(), seq)
        out[name] = {"pods": bits(flags), "checked": checked, "skipped": skipped, "E": f.dims["E"], "seq": [int(x) for x in seq],
                     "device_agrees": bool(np.array_equal(flags, dev["pod_flags"]) and dev["checked"] == dict(zip(TR.RULES, checked)) and dev["skipped_groups"] == skipped)}
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
rr_cases, pack_cases, order_cases = json.loads(sys.argv[1])
def problem(kind, args):
    return R.rr_problem(args["seed"]) if kind == "rr" else T.mid_problem_wide(args["seed"]) if kind == "wide" else (getattr(W, kind)(**args) if kind != "mid" else T.mid_problem(args["seed"]))
for name, kind, args in rr_cases:
    f = S.FlatProblem(problem(kind, args)); f.solve(decode=False); audited("rr/" + name, f); f.close()
for name, kind, args, no_rr in pack_cases:
    f = S.FlatProblem(E._problem(kind, args), flags=S.KS_FLAG_NO_RR if no_rr else 0); f.solve(decode=False); audited("pack/" + name, f); f.close()
for name, kind, args in order_cases:      # the commit-order gate's problems, through ks_pack as well (ks_pack_rr's numbers are above)
    f = S.FlatProblem(problem(kind, args), flags=S.KS_FLAG_NO_RR); f.solve(decode=False); audited("order/" + name, f); f.close()
its, prov, nodes, bound = W.cluster_snapshot(existing=24, sizes=5, seed=11)
snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
flats = S.open_whatifs(snap, pn, [[0, 3], [5], [1, 2, 9], [7, 11]], derive=False)
for f in flats: f.upload(0)
S.solve_batch(flats, decode=False)
for i, f in enumerate(flats): audited("whatifs/%%d" %% i, f)
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
parsed = S.ParsedProblem(snap)
flats = S.open_whatifs(parsed, pod_node, E.WIDE_SETS, derive=False)
S.solve_batch(flats, decode=False)
for i, f in enumerate(flats): audited("wide_whatifs/%%d" %% i, f)
plain = [out["wide_whatifs/%%d" %% i] for i in range(len(flats))]
# derived on the device: no flattening of their own to restate the pass over -- the device pass of the batch, which must find what the reference found above: nothing
derived = S.open_whatifs(parsed, pod_node, E.WIDE_SETS, derive=True)
S.solve_batch_resident(derived)
for i, d in enumerate(S.audit_topology_batch(derived)):
    out["wide_whatifs_derived/%%d" %% i] = {"pods": bits(d["pod_flags"]), "checked": [d["checked"][k] for k in TR.RULES], "skipped": d["skipped_groups"], "device_agrees": True}
for name, mk in (("leaders and followers", TC.leaders_and_followers), ("a key of 64 values", TC.racks), ("24 groups", TC.many_groups), ("P = 1", lambda: TC.plain(1)),
                 ("n_new = 0 and G = 0", lambda: TC.plain(3, True))):
    for no_rr in (False, True):
        f = S.FlatProblem(mk(), flags=S.KS_FLAG_NO_RR if no_rr else 0); f.solve(decode=False); audited("shape/%%s/%%d" %% (name, no_rr), f)
        out["shape/%%s/%%d" %% (name, no_rr)]["n_new"] = int(f.result_arrays()["n_new"]); f.close()
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in TC.run_tamper_matrix(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)] for n, ok in TC.run_shape_tampers(S)]
print("RESULT " + json.dumps(out))
"""

# problems without existing nodes that both pack kernels run on the emulator: topology over the zone and the hostname, RUN rounds (config3), the head window, relaxation
ORDER_CASES = [c for c in E.CASES if c[0] in ("config3_140", "config3_700", "mid_0", "herd_600")]
NAMES = ["rr/" + c[0] for c in E.CASES] + ["pack/" + c[0] for c in E.PACK_CASES] + ["whatifs/%d" % i for i in range(4)] + \
        ["wide_whatifs/%d" % i for i in range(len(E.WIDE_SETS))] + ["wide_whatifs_derived/%d" % i for i in range(len(E.WIDE_SETS))]
SHAPES = ["leaders and followers", "a key of 64 values", "24 groups", "P = 1", "n_new = 0 and G = 0"]


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [E.CASES, E.PACK_CASES, ORDER_CASES])


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["pods"] == {}, got["pods"]
    assert got["device_agrees"], got


def test_the_gate_is_not_vacuous(emulated):
    """Over the committed cases every rule evaluated something: the clean results above were not clean for lack of anything to check."""
    total = [sum(emulated[n]["checked"][i] for n in NAMES) for i in range(4)]
    assert all(t > 0 for t in total), total
    assert emulated["rr/config3_3500"]["checked"][0] > 3000 and sum(emulated[n]["checked"][1] for n in NAMES) > 100


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("no_rr", [0, 1], ids=["ks_pack_rr", "ks_pack"])
def test_hand_made_problems_are_solved_clean_on_the_emulator(emulated, name, no_rr):
    got = emulated["shape/%s/%d" % (name, no_rr)]
    assert "error" not in got, got
    assert got["pods"] == {} and got["device_agrees"], got
    if name == "leaders and followers":
        assert got["checked"][2] == 8, got      # four followers on the hostname, four on the zone
    if name == "24 groups":
        assert got["checked"][1] >= 24, got
    if name == "n_new = 0 and G = 0":
        assert got["n_new"] == 0 and got["checked"] == [3, 0, 0, 0] and got["skipped"] == 0, got
    if name == "P = 1":
        assert got["checked"] == [1, 0, 0, 0], got


@pytest.mark.parametrize("i", range(len(TC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    """tests/audit_topo_cases.py: one minimal edit per rule and direction through the claimed form -- exactly that bit on exactly those pods, from the kernels' source and from the reference."""
    name, ok = emulated["tamper"][i]
    assert name == TC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(TC.SHAPE_TAMPER_NAMES)))
def test_violations_at_the_kernels_edges_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == TC.SHAPE_TAMPER_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the commit-order gate
ORACLE_CHILD = r"""
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import json
from karpenter_core_amd import workloads as W
from oracle import oracle_py
import test_fuzz_mid as T
kind, args = json.loads(sys.argv[1])
p = getattr(W, kind)(**args) if kind != "mid" else T.mid_problem(args["seed"])
oracle_py.solve(p)
"""


_ORACLE_ORDER = {}      # case -> the oracle's commit order: one oracle run per problem, shared by the two kernels' tests


def _oracle_commit_order(kind, args):
    key = json.dumps([kind, args], sort_keys=True)
    if key not in _ORACLE_ORDER:
        _ORACLE_ORDER[key] = _trace_commit_order(kind, args)
    return _ORACLE_ORDER[key]


def _trace_commit_order(kind, args):
    """The pods in the order of their successful Scheduler.add, from the oracle's KO_TRACE file (written when the process ends: a process per problem).  A line is
    `pod position ...`: position >= 0 -- the open node that took the pod; -1 -- no open node did and the templates are tried, which can fail (the pod is then relaxed
    and comes back).  A pod that ended up placed succeeded at its last line."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace")
        env = dict(os.environ, KO_TRACE=path)
        pr = subprocess.run([sys.executable, "-c", ORACLE_CHILD % {"root": ROOT, "tests": HERE}, json.dumps([kind, args])], capture_output=True, text=True, env=env, timeout=600)
        assert pr.returncode == 0, pr.stderr[-2000:]
        last = {}
        for i, line in enumerate(open(path)):
            last[int(line.split()[0])] = i
    return [p for p, _ in sorted(last.items(), key=lambda kv: kv[1])]


@pytest.mark.parametrize("kernel", ["rr", "order"], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name,kind,args", ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_pod_seq_is_the_references_commit_order_across_nodes(emulated, name, kind, args, kernel):
    got = emulated[kernel + "/" + name]
    assert "error" not in got, got
    assert got["E"] == 0, "the trace has no line for a pod an existing node took"
    seq = np.array(got["seq"])
    placed = np.nonzero(seq >= 0)[0]
    ours = [int(p) for p in placed[np.argsort(seq[placed], kind="stable")]]
    assert sorted(seq[placed]) == list(range(len(placed)))
    theirs = [p for p in _oracle_commit_order(kind, args) if seq[p] >= 0]
    assert len(theirs) == len(ours)
    first = next((i for i, (a, b) in enumerate(zip(ours, theirs)) if a != b), None)
    assert first is None, (first, ours[first:first + 8], theirs[first:first + 8])


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
def _tiny():
    """One narrow key (the zone: values 0, 1; well known), one template that leaves it open, two existing nodes (e0 in zone 0, e1 without the label), six groups:
       g0 anti-affinity over the hostname   g1 anti-affinity over the zone   g2 affinity over the hostname   g3 affinity over the zone
       g4 hostname spread, maxSkew 1, no filter term   g5 anti-affinity over the zone, created by a later Topology.Update (grp_active 0)
    and classes:  0 plain | 1 owns g0 and is selected by it | 2 owns g1 and is selected by it | 3 leader: selected by g2 and g3 | 4 owns g2 | 5 owns g3 |
       6 owns g4, self-selecting, selected by it | 7 selected by g1 only (constrained by nothing) | 8 owns g3, self-selecting | 9 owns g5 and is selected by it.
    Eight pods, all of class 0 until a case says otherwise, on existing node e0 in commit order 0 .. 7."""
    u32, u64, i32 = (lambda *x: np.array(x, dtype=np.uint32)), (lambda *x: np.array(x, dtype=np.uint64)), (lambda *x: np.array(x, dtype=np.int32))
    SELF = 1 << 31
    own = [[], [0 | SELF], [1 | SELF], [], [2], [3], [4 | SELF], [], [3 | SELF], [5 | SELF]]
    sel = [[], [0], [1], [2, 3], [], [], [4], [1], [3], [5]]
    off = lambda ls: np.cumsum([0] + [len(x) for x in ls]).astype(np.uint32)
    flat = lambda ls: np.array([x for l in ls for x in l], dtype=np.uint32)
    C, Pn = len(own), 8
    p = {"P": Pn, "C": C, "M": 1, "E": 2, "K": 1, "G": 6, "GH": 3, "wellknown_mask": 1, "key_nvalues": u32(2), "value_int": np.full(64, -2 ** 31, dtype=np.int32),
         "pod_stage_off": np.arange(Pn + 1, dtype=np.uint32), "stage_cls": np.zeros(Pn, dtype=np.uint32),
         "cls_own_off": off(own), "own_list": flat(own), "cls_sel_off": off(sel), "sel_list": flat(sel), "cls_isel_off": np.zeros(C + 1, dtype=np.uint32), "isel_list": u32(),
         "cls_iown_off": np.zeros(C + 1, dtype=np.uint32), "iown_list": u32(),
         "grp_type": np.array([2, 2, 1, 1, 0, 2], dtype=np.uint8), "grp_key": i32(-2, 0, -2, 0, -2, 0), "grp_active": np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8),
         "grp_max_skew": i32(0, 0, 0, 0, 1, 0), "grp_hslot": i32(0, -1, 1, -1, 2, -1), "grp_count": np.zeros(6 * 64, dtype=np.int32), "grph_count": np.zeros(3 * 2, dtype=np.int32),
         "grp_filter_off": u32(0, 0, 0, 0, 0, 0, 0), "flt.present": u32(), "flt.it_state": i32()}
    for fam, n, present, mask in (("tmpl", 1, [0], [0]), ("en", 2, [1, 0], [1, 0]), ("cls", C, [0] * C, [0] * C)):
        p.update({fam + ".present": np.array(present, dtype=np.uint32), fam + ".complement": np.zeros(n, dtype=np.uint32), fam + ".mask": np.array(mask, dtype=np.uint64),
                  fam + ".gt": np.full(n, A.NOGT, dtype=np.int32), fam + ".lt": np.full(n, A.NOLT, dtype=np.int32), fam + ".it_state": np.zeros(n, dtype=np.int32)})
    r = {"n_existing": 2, "n_new": 2, "pod_node": np.zeros(Pn, dtype=np.int32), "pod_stage": np.zeros(Pn, dtype=np.int32), "unscheduled": i32(), "node_tmpl": i32(0, 0),
         "node_present": u32(1, 0), "node_complement": u32(0, 0), "node_mask": u64(2, 0).reshape(2, 1), "node_gt": np.full((2, 1), A.NOGT, dtype=np.int32),
         "node_lt": np.full((2, 1), A.NOLT, dtype=np.int32)}      # new node 0 (index 2) is in zone 1; new node 1 (index 3) never got the key
    return p, r, np.arange(Pn, dtype=np.int32)


E0, E1, N0, N1 = 0, 1, 2, 3
AA, AF, HS, SQ = TR.BITS["ANTI_AFFINITY"], TR.BITS["AFFINITY"], TR.BITS["HOSTNAME_SPREAD"], TR.BITS["SEQ"]


def _unit(name):
    p, r, s = _tiny()
    cls, node = p["stage_cls"], r["pod_node"]
    want = {}
    if name == "clean":
        pass
    elif name == "hostname anti-affinity: the later pod":
        cls[0] = cls[1] = 1; want = {1: AA}
    elif name == "hostname anti-affinity: the commit numbers swapped":
        cls[0] = cls[1] = 1; s[0], s[1] = 1, 0; want = {0: AA}
    elif name == "hostname anti-affinity: different nodes":
        cls[0] = cls[1] = 1; node[1] = N0
    elif name == "hostname anti-affinity: the node's initial count":
        cls[0] = 1; p["grph_count"][0 * 2 + E0] = 1; want = {0: AA}
    elif name == "hostname anti-affinity: an unregistered hostname counts nothing":
        cls[0] = 1; p["grph_count"][0 * 2 + E0] = -1
    elif name == "zone anti-affinity: an earlier certain recorder on another node":
        cls[0] = cls[1] = 2; node[1] = N0; p["en.mask"][E0] = 2; want = {1: AA}      # e0 relabelled to zone 1, where new node 0 is
    elif name == "zone anti-affinity: the recorder is later":
        cls[0] = cls[1] = 2; node[1] = N0; p["en.mask"][E0] = 2; s[0], s[1] = 1, 0; want = {0: AA}
    elif name == "zone anti-affinity: different zones":
        cls[0] = cls[1] = 2; node[1] = N0
    elif name == "zone anti-affinity: an uncertain recorder is not believed":
        cls[0] = 7; cls[1] = 2; node[0] = N0; node[1] = E0; p["en.mask"][E0] = 2      # class 7 is selected by g1 and constrained by nothing: its machine got the zone from a later pod
    elif name == "zone anti-affinity: the same recorder made certain by its class":
        cls[0] = 7; cls[1] = 2; node[0] = N0; node[1] = E0; p["en.mask"][E0] = 2; p["cls.present"][7] = 1; p["cls.mask"][7] = 2; want = {1: AA}
    elif name == "zone anti-affinity: the initial count":
        cls[0] = 2; p["grp_count"][1 * 64 + 0] = 3; want = {0: AA}
    elif name == "zone anti-affinity: a node that is not concrete":
        cls[0] = 2; node[0] = N1; want = {0: AA}
    elif name == "zone anti-affinity: an existing node without the well-known label is not examined":
        cls[0] = 2; node[0] = E1
    elif name == "hostname affinity: no leader on the node":
        cls[0] = 3; cls[1] = 4; node[1] = E1; want = {1: AF}
    elif name == "hostname affinity: the leader is there":
        cls[0] = 3; cls[1] = 4
    elif name == "hostname affinity: the leader came later":
        cls[0] = 3; cls[1] = 4; s[0], s[1] = 1, 0; want = {1: AF}
    elif name == "hostname affinity: the node's initial count":
        cls[1] = 4; p["grph_count"][1 * 2 + E0] = 2
    elif name == "zone affinity: no leader in the zone":
        cls[0] = 3; cls[1] = 5; node[1] = N0; want = {1: AF}
    elif name == "zone affinity: a leader on another node of the zone":
        cls[0] = 3; cls[1] = 5; node[0] = N0; p["en.mask"][E0] = 2
    elif name == "zone affinity: an uncertain recorder is believed":
        cls[0] = 3; cls[1] = 5; node[0] = N1      # the leader's machine never got the key: it Has every zone
    elif name == "zone affinity: the leader came later":
        cls[0] = 3; cls[1] = 5; s[0], s[1] = 1, 0; want = {1: AF}
    elif name == "zone affinity: the initial count":
        cls[1] = 5; p["grp_count"][3 * 64 + 0] = 1
    elif name == "zone affinity: self-selecting is not examined":
        cls[1] = 8; node[1] = N0
    elif name == "hostname spread: one owner too many":
        cls[0] = cls[1] = cls[2] = 6; p["grp_max_skew"][4] = 2; want = {2: HS}
    elif name == "hostname spread: within the skew":
        cls[0] = cls[1] = 6; p["grp_max_skew"][4] = 2
    elif name == "hostname spread: the node's initial count":
        cls[0] = 6; p["grph_count"][2 * 2 + E0] = 1; want = {0: HS}
    elif name == "hostname spread: under a node filter it is not examined":
        cls[0] = cls[1] = 6; p["grp_filter_off"][5:] = 1; p["flt.present"] = np.array([1], dtype=np.uint32); p["flt.it_state"] = np.array([0], dtype=np.int32)
    elif name == "hostname spread: a filter term that requires nothing is no filter":
        cls[0] = cls[1] = 6; p["grp_filter_off"][5:] = 1; p["flt.present"] = np.array([0], dtype=np.uint32); p["flt.it_state"] = np.array([0], dtype=np.int32); want = {1: HS}
    elif name == "a group created later is skipped":
        cls[0] = cls[1] = 9
    elif name == "SEQ: two pods with one commit number":
        cls[0] = cls[1] = 1; s[1] = 0; want = {0: SQ, 1: SQ}      # (and neither is examined further: the anti-affinity between them goes unflagged)
    elif name == "SEQ: a commit number past the placed pods":
        s[7] = 8; want = {7: SQ}
    elif name == "SEQ: an unscheduled pod's number is not this pass's":
        node[7] = -1; s[7] = -1
    else:
        raise KeyError(name)
    return p, r, s, want


UNIT = ["clean", "hostname anti-affinity: the later pod", "hostname anti-affinity: the commit numbers swapped", "hostname anti-affinity: different nodes",
        "hostname anti-affinity: the node's initial count", "hostname anti-affinity: an unregistered hostname counts nothing",
        "zone anti-affinity: an earlier certain recorder on another node", "zone anti-affinity: the recorder is later", "zone anti-affinity: different zones",
        "zone anti-affinity: an uncertain recorder is not believed", "zone anti-affinity: the same recorder made certain by its class", "zone anti-affinity: the initial count",
        "zone anti-affinity: a node that is not concrete", "zone anti-affinity: an existing node without the well-known label is not examined",
        "hostname affinity: no leader on the node", "hostname affinity: the leader is there", "hostname affinity: the leader came later", "hostname affinity: the node's initial count",
        "zone affinity: no leader in the zone", "zone affinity: a leader on another node of the zone", "zone affinity: an uncertain recorder is believed",
        "zone affinity: the leader came later", "zone affinity: the initial count", "zone affinity: self-selecting is not examined",
        "hostname spread: one owner too many", "hostname spread: within the skew", "hostname spread: the node's initial count",
        "hostname spread: under a node filter it is not examined", "hostname spread: a filter term that requires nothing is no filter", "a group created later is skipped",
        "SEQ: two pods with one commit number", "SEQ: a commit number past the placed pods", "SEQ: an unscheduled pod's number is not this pass's"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, want = _unit(name)
    flags, checked, skipped = TR.audit(p, r, s)
    assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == want
    assert skipped == 1
    if name == "a group created later is skipped":
        assert checked[1:] == [0, 0, 0]
    if "not examined" in name:
        assert checked[1:] == [0, 0, 0], checked


def test_every_bit_has_a_unit_case_in_both_directions():
    raised, clean = 0, 0
    for name in UNIT:
        want = _unit(name)[3]
        for b in want.values():
            raised |= b
        if not want:
            clean += 1
    assert raised == sum(TR.BITS.values()) and clean >= 10
