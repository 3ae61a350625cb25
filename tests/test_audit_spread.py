"""(CPU) The audit's third pass -- topology spread over narrow keys in commit order (include/ksolve.h ks_audit_spread_dev, KS_AUDIT_POD_SPREAD) -- validated where a
correct result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_spread_ref.py) over every result the lane-fibre emulator returns for its committed cases -- the set
     tests/test_audit_topology.py audits, results proven equal to the oracle's in tests/test_rr_emulated.py -- and over the what-ifs of
     tests/test_whatif_derived.py's decorated snapshot raises NO flag; a rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source
     (karpenter_core_amd/csrc/ks_audit_spread.inc) is compiled into the emulator build and runs beside the reference: the two agree bit for bit, `checked` and
     `exact_pairs` included.  Over the set the rule examined pairs, and some of them exactly;
  b) the tamper matrix and the kernels' other paths (tests/audit_spread_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause of the rule and per direction.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import numpy as np
import pytest

import audit_harness as H
import audit_ref as A
import audit_spread_cases as SC
import audit_spread_ref as SR
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
import audit_spread_ref as SR, audit_spread_cases as SC
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR, test_whatif_derived as WD
out = {}
def audited(name, f):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev, flags = SC.compare(S, f)
        out[name] = dict(SC.summary(dev), device_agrees=True)
    except AssertionError as e:
        out[name] = {"error": "device and reference differ: " + str(e)[:300]}
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
rr_cases, pack_cases = json.loads(sys.argv[1])
def problem(kind, args):
    return R.rr_problem(args["seed"]) if kind == "rr" else T.mid_problem_wide(args["seed"]) if kind == "wide" else (getattr(W, kind)(**args) if kind != "mid" else T.mid_problem(args["seed"]))
for name, kind, args in rr_cases:
    f = S.FlatProblem(problem(kind, args)); f.solve(decode=False); audited("rr/" + name, f); f.close()
    f = S.FlatProblem(problem(kind, args), flags=S.KS_FLAG_NO_RR); f.solve(decode=False); audited("no_rr/" + name, f); f.close()
for name, kind, args, no_rr in pack_cases:
    f = S.FlatProblem(E._problem(kind, args), flags=S.KS_FLAG_NO_RR if no_rr else 0); f.solve(decode=False); audited("pack/" + name, f); f.close()
its, prov, nodes, bound = W.cluster_snapshot(existing=24, sizes=5, seed=11)
snap, pn = W.snapshot_problem(its, prov, nodes, bound, False)
flats = S.open_whatifs(snap, pn, [[0, 3], [5], [1, 2, 9], [7, 11]], derive=False)
for f in flats: f.upload(0)
S.solve_batch(flats, decode=False)
for i, f in enumerate(flats): audited("whatifs/%%d" %% i, f)
def both_forms(tag, parsed, pod_node, sets):
    flats = S.open_whatifs(parsed, pod_node, sets, derive=False)
    S.solve_batch(flats, decode=False)
    for i, f in enumerate(flats): audited(tag + "/%%d" %% i, f)
    # derived on the device: no flattening of their own to restate the pass over -- the device pass of the batch, which must find what the reference found above
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True)
    S.solve_batch_resident(derived)
    whole = S.audit_spread_batch(derived)
    for i, d in enumerate(whole):
        out[tag + "_derived/%%d" %% i] = dict(SC.summary(d), device_agrees=True)
    try:
        out[tag + "_sliced"] = SC.sliced_batch_says_the_same(S, derived, whole)
    except AssertionError as e:
        out[tag + "_sliced"] = str(e)[:300]
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
both_forms("wide_whatifs", S.ParsedProblem(snap), pod_node, E.WIDE_SETS)
its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
both_forms("topology_whatifs", S.ParsedProblem(snap), pod_node, json.loads(sys.argv[2]))
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in SC.run_tamper_matrix(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)] for n, ok in SC.run_shapes(S)]
print("RESULT " + json.dumps(out))
"""

TOPOLOGY_SETS = H.WHATIF_SETS
WHATIFS, FLAT, DERIVED = H.gate_names()
NAMES = FLAT + DERIVED


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [E.CASES, E.PACK_CASES], TOPOLOGY_SETS)


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["pods"] == {}, got["pods"]
    assert got["device_agrees"], got


def test_the_gate_is_not_vacuous(emulated):
    """Over the committed cases the rule examined pairs, and some of them exactly: the clean results above were not clean for lack of anything to check."""
    pairs, exact = sum(emulated[n]["checked"][1] for n in FLAT), sum(emulated[n]["exact"] for n in FLAT)
    print(pairs, exact)
    assert pairs > 1000 and exact > 0, (pairs, exact)
    assert sum(emulated[n]["checked"][1] for n in FLAT if n.startswith("topology_whatifs/")) > 0


@pytest.mark.parametrize("name", DERIVED)
def test_a_derived_whatif_counts_what_the_same_whatif_flattened_counts(emulated, name):
    """The batch form over what-ifs derived on the device -- their own group tables, the results where they lie -- examines as many pods and pairs, as many of them
    exactly, as the reference does over the same what-if flattened.  (The groups are the snapshot's in a derived what-if: the unattempted ones are not compared.)"""
    d, p = emulated[name], emulated[name.replace("_derived", "")]
    assert (d["checked"], d["exact"], d["n_new"], d["n_placed"]) == (p["checked"], p["exact"], p["n_new"], p["n_placed"]), (d, p)


@pytest.mark.parametrize("tag", ["wide_whatifs", "topology_whatifs"])
def test_a_batch_walked_in_slices_says_what_it_said_in_one(emulated, tag):
    assert emulated[tag + "_sliced"] is True, emulated[tag + "_sliced"]


@pytest.mark.parametrize("i", range(len(SC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    """tests/audit_spread_cases.py: each edit through the claimed form raises its bit on exactly the pods it names, from the kernels' source and from the reference."""
    name, ok = emulated["tamper"][i]
    assert name == SC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(SC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == SC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
def _tiny():
    """One narrow key (the zone, well known: values 0 1 2 registered, value 3 known and not registered), two templates (0 leaves the zone open, 1 names zone 1), three
    existing nodes (e0 in zone 0, e1 in zone 1, e2 without the label), four new nodes (n0: template 0, ended in zone 0 | n1: template 1, zone 1 | n2: template 0,
    ended with zones 0 and 1 | n3: template 0, never got the key) and four spread groups:
       g0 over the zone, maxSkew 1, no filter   g1 the same under a node filter   g2 the same, created by a later Topology.Update   g3 over the hostname
    Classes:  0 plain | 1 owns g0, self-selecting, selected by it | 2 owns g0, not selected | 3 selected by g0 only (a recorder constrained by nothing) |
       4 as 1, requires zone In {0, 1} | 5 as 1, requires zone In {3} | 6 owns g1 and is selected by it | 7 owns g2 and is selected by it | 8 plain, requires zone In {0}.
    Eight pods, all of class 0 until a case says otherwise, on e0 in commit order 0 .. 7."""
    u32, u64, i32 = (lambda *x: np.array(x, dtype=np.uint32)), (lambda *x: np.array(x, dtype=np.uint64)), (lambda *x: np.array(x, dtype=np.int32))
    SELF = 1 << 31
    own = [[], [0 | SELF], [0], [], [0 | SELF], [0 | SELF], [1 | SELF], [2 | SELF], []]
    sel = [[], [0], [], [0], [0], [0], [1], [2], []]
    off = lambda ls: np.cumsum([0] + [len(x) for x in ls]).astype(np.uint32)
    flat = lambda ls: np.array([x for l in ls for x in l], dtype=np.uint32)
    C, Pn = len(own), 8
    count = np.full(4 * 64, -1, dtype=np.int32)
    for g in range(3):
        count[g * 64:g * 64 + 3] = 0
    p = {"P": Pn, "C": C, "M": 2, "E": 3, "K": 1, "G": 4, "GH": 1, "wellknown_mask": 1, "key_nvalues": u32(4), "value_int": np.full(64, -2 ** 31, dtype=np.int32),
         "pod_stage_off": np.arange(Pn + 1, dtype=np.uint32), "stage_cls": np.zeros(Pn, dtype=np.uint32),
         "cls_own_off": off(own), "own_list": flat(own), "cls_sel_off": off(sel), "sel_list": flat(sel), "cls_isel_off": np.zeros(C + 1, dtype=np.uint32), "isel_list": u32(),
         "cls_iown_off": np.zeros(C + 1, dtype=np.uint32), "iown_list": u32(),
         "grp_type": np.zeros(4, dtype=np.uint8), "grp_key": i32(0, 0, 0, -2), "grp_active": np.array([1, 1, 0, 1], dtype=np.uint8), "grp_max_skew": i32(1, 1, 1, 1),
         "grp_hslot": i32(-1, -1, -1, 0), "grp_count": count, "grph_count": np.zeros(3, dtype=np.int32),
         "grp_filter_off": u32(0, 0, 1, 1, 1), "flt.present": u32(1), "flt.it_state": i32(0)}
    cls_present, cls_mask = [0] * C, [0] * C
    cls_present[4], cls_mask[4] = 1, 0b0011
    cls_present[5], cls_mask[5] = 1, 0b1000
    cls_present[8], cls_mask[8] = 1, 0b0001
    for fam, n, present, mask in (("tmpl", 2, [0, 1], [0, 2]), ("en", 3, [1, 1, 0], [1, 2, 0]), ("cls", C, cls_present, cls_mask)):
        p.update({fam + ".present": np.array(present, dtype=np.uint32), fam + ".complement": np.zeros(n, dtype=np.uint32), fam + ".mask": np.array(mask, dtype=np.uint64),
                  fam + ".gt": np.full(n, A.NOGT, dtype=np.int32), fam + ".lt": np.full(n, A.NOLT, dtype=np.int32), fam + ".it_state": np.zeros(n, dtype=np.int32)})
    r = {"n_existing": 3, "n_new": 4, "pod_node": np.zeros(Pn, dtype=np.int32), "pod_stage": np.zeros(Pn, dtype=np.int32), "unscheduled": i32(), "node_tmpl": i32(0, 1, 0, 0),
         "node_present": u32(1, 1, 1, 0), "node_complement": u32(0, 0, 0, 0), "node_mask": u64(1, 2, 3, 0).reshape(4, 1), "node_gt": np.full((4, 1), A.NOGT, dtype=np.int32),
         "node_lt": np.full((4, 1), A.NOLT, dtype=np.int32)}
    return p, r, np.arange(Pn, dtype=np.int32)


E0, E1, E2, N0, N1, N2, N3 = range(7)
SP, SQ = SR.BITS["SPREAD"], SR.BITS["SEQ"]
OWNER, OWNER_NOT_SELF, RECORDER, OWNER_Z01, OWNER_Z3, FILTERED, LATE, PINNER = 1, 2, 3, 4, 5, 6, 7, 8


def _unit(name):
    """(problem, result, commit numbers, {pod: bits}, pairs examined, of them exact)"""
    p, r, s = _tiny()
    cls, node, init = p["stage_cls"], r["pod_node"], p["grp_count"]
    want, pairs, exact = {}, None, None
    if name == "clean":
        pairs = 0
    elif name == "an earlier recorder counts":
        cls[0] = RECORDER; cls[1] = OWNER; want = {1: SP}; pairs, exact = 1, 1      # zone 0 at 1 0 0: 1 + 1 - 0 > 1
    elif name == "a later recorder does not":
        cls[0] = RECORDER; cls[1] = OWNER; s[0], s[1] = 1, 0; pairs, exact = 1, 1
    elif name == "certain by the existing node's label":
        cls[0] = RECORDER; cls[1] = OWNER; node[0] = E1; node[1] = E1; want = {1: SP}; pairs, exact = 1, 1
    elif name == "certain by the template's single value":
        cls[0] = RECORDER; cls[1] = OWNER; node[0] = N1; node[1] = E1; want = {1: SP}; pairs, exact = 1, 1
    elif name == "certain by pin time: the pinning pod is earlier than the recorder":
        cls[2] = PINNER; cls[0] = RECORDER; cls[1] = OWNER; node[2] = node[0] = N0; s[2], s[0], s[1] = 0, 1, 2; want = {1: SP}; pairs, exact = 1, 1
    elif name == "not certain: the pinning pod is later than the recorder":
        cls[2] = PINNER; cls[0] = RECORDER; cls[1] = OWNER; node[2] = node[0] = N0; s[0], s[2], s[1] = 0, 1, 2; pairs, exact = 1, 0
    elif name == "a pod that owns a spread group on the key pins its node itself":
        cls[0] = cls[1] = OWNER; node[0] = N0; want = {1: SP}; pairs, exact = 2, 2      # pod 0 on the machine it opened: its own topology requirement was one zone
    elif name == "without the recorder the emptiest zone is empty":
        cls[1] = OWNER; node[1] = E1; init[0:3] = [0, 1, 9]; want = {1: SP}; pairs, exact = 1, 1      # zone 1 at 0 1 9: 1 + 1 - 0 > 1
    elif name == "an uncertain recorder raises U only: the minimum":
        cls[0] = RECORDER; node[0] = N0; cls[1] = OWNER; node[1] = E1; init[0:3] = [0, 1, 9]; pairs, exact = 1, 0      # zone 0 may hold one: 1 + 1 - 1
    elif name == "an uncertain recorder raises U only: not the pod's own count":
        cls[0] = RECORDER; node[0] = N0; cls[1] = OWNER; pairs, exact = 1, 0      # the same recorder, certain, flags pod 1 ("an earlier recorder counts")
    elif name == "a wild recorder raises every minimum":
        cls[0] = RECORDER; node[0] = E2; cls[1] = OWNER; node[1] = E1; init[0:3] = [0, 1, 9]; pairs, exact = 1, 0
    elif name == "self 0: the pod does not count itself":
        cls[0] = RECORDER; cls[1] = OWNER_NOT_SELF; pairs, exact = 1, 1      # 1 + 0 - 0
    elif name == "the whole universe: the empty zone is the minimum":
        cls[0] = OWNER; init[0:3] = [1, 1, 0]; want = {0: SP}; pairs, exact = 1, 1
    elif name == "a class requirement excludes the emptiest zone from the minimum":
        cls[0] = OWNER_Z01; init[0:3] = [1, 1, 0]; pairs, exact = 1, 1
    elif name == "a class requirement that leaves no registered zone in the minimum":
        cls[0] = OWNER_Z3; init[0:3] = [5, 0, 0]; pairs, exact = 1, 1
    elif name == "the pod's zone is not registered":
        cls[0] = OWNER; init[0] = -1; want = {0: SP}; pairs, exact = 1, 0
    elif name == "a final set of two values":
        cls[0] = OWNER; node[0] = N2; want = {0: SP}; pairs, exact = 1, 0
    elif name == "a new node that never got the key":
        cls[0] = OWNER; node[0] = N3; want = {0: SP}; pairs, exact = 1, 0
    elif name == "an existing node without the well-known label is not examined":
        cls[0] = cls[1] = cls[2] = OWNER; node[0] = node[1] = node[2] = E2; pairs = 0
    elif name == "a filtered group and a late group are skipped":
        cls[0] = cls[1] = cls[2] = FILTERED; cls[3] = cls[4] = cls[5] = LATE; pairs = 0
    elif name == "a pod that fails SEQ is unplaced: it records nothing":
        cls[0] = RECORDER; cls[1] = OWNER; s[2] = 0; want = {0: SQ, 2: SQ}; pairs, exact = 1, 1
    else:
        raise KeyError(name)
    return p, r, s, want, pairs, exact


UNIT = ["clean", "an earlier recorder counts", "a later recorder does not", "certain by the existing node's label", "certain by the template's single value",
        "certain by pin time: the pinning pod is earlier than the recorder", "not certain: the pinning pod is later than the recorder",
        "a pod that owns a spread group on the key pins its node itself", "without the recorder the emptiest zone is empty", "an uncertain recorder raises U only: the minimum",
        "an uncertain recorder raises U only: not the pod's own count", "a wild recorder raises every minimum", "self 0: the pod does not count itself",
        "the whole universe: the empty zone is the minimum", "a class requirement excludes the emptiest zone from the minimum",
        "a class requirement that leaves no registered zone in the minimum", "the pod's zone is not registered", "a final set of two values", "a new node that never got the key",
        "an existing node without the well-known label is not examined", "a filtered group and a late group are skipped", "a pod that fails SEQ is unplaced: it records nothing"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, want, pairs, exact = _unit(name)
    flags, checked, got_exact, skipped = SR.audit(p, r, s)
    assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == want
    assert skipped == 3 and checked[0] == 8      # g1 (filtered), g2 (late) and g3 (the hostname) are unattempted
    assert checked[1] == pairs and got_exact == (exact or 0), (checked, got_exact)


def test_both_directions_have_unit_cases():
    flagged = [n for n in UNIT if SP in _unit(n)[3].values()]
    assert len(flagged) >= 8 and len(UNIT) - len(flagged) >= 10
