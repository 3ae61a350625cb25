"""(CPU) The audit's fourth pass -- first-fit order from the final state and the commit numbers (include/ksolve.h ks_audit_firstfit_dev, KS_AUDIT_POD_FIT_*) --
validated where a correct result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_firstfit_ref.py) over every result the lane-fibre emulator returns for its committed cases -- the set
     tests/test_audit_spread.py audits, results proven equal to the oracle's in tests/test_rr_emulated.py -- and over the what-ifs of tests/test_whatif_derived.py's
     decorated snapshot raises NO flag; a rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source
     (karpenter_core_amd/csrc/ks_audit_firstfit.inc) is compiled into the emulator build and runs beside the reference: the two agree bit for bit, `checked`,
     `admitting_pairs` and `skipped_pods` included.  Over the set the rule examined pods, and some (class, node) pairs admitted;
  b) the tamper matrix and the kernels' other paths (tests/audit_firstfit_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause of the rule and per direction.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import audit_ref as A
import audit_firstfit_cases as FC
import audit_firstfit_ref as FR
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
import audit_firstfit_ref as FR, audit_firstfit_cases as FC
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR, test_whatif_derived as WD
out = {}
def audited(name, f):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev, flags = FC.compare(S, f)
        out[name] = dict(FC.summary(dev), device_agrees=True)
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
    for i, d in enumerate(S.audit_firstfit_batch(derived)):
        out[tag + "_derived/%%d" %% i] = dict(FC.summary(d), device_agrees=True)
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
both_forms("wide_whatifs", S.ParsedProblem(snap), pod_node, E.WIDE_SETS)
its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
both_forms("topology_whatifs", S.ParsedProblem(snap), pod_node, json.loads(sys.argv[2]))
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in FC.run_tamper_matrix(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)] for n, ok in FC.run_shapes(S)]
print("RESULT " + json.dumps(out))
"""

TOPOLOGY_SETS = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]
WHATIFS = ["whatifs/%d" % i for i in range(4)] + ["wide_whatifs/%d" % i for i in range(len(E.WIDE_SETS))] + ["topology_whatifs/%d" % i for i in range(len(TOPOLOGY_SETS))]
FLAT = ["rr/" + c[0] for c in E.CASES] + ["no_rr/" + c[0] for c in E.CASES] + ["pack/" + c[0] for c in E.PACK_CASES] + WHATIFS
DERIVED = ["wide_whatifs_derived/%d" % i for i in range(len(E.WIDE_SETS))] + ["topology_whatifs_derived/%d" % i for i in range(len(TOPOLOGY_SETS))]
NAMES = FLAT + DERIVED


@pytest.fixture(scope="module")
def emulated():
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None); env.pop("KS_NO_RR", None)
    env["KS_SIM_ALARM"] = "600"
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, json.dumps([E.CASES, E.PACK_CASES]), json.dumps(TOPOLOGY_SETS)], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, pr.stdout[-2000:] + pr.stderr[-2000:]
    return json.loads(line[-1][7:])


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["pods"] == {}, got["pods"]
    assert got["device_agrees"], got


def test_the_gate_is_not_vacuous(emulated):
    """Over the committed cases the rule examined pods and found (class, node) pairs that admit -- the clean results above were not clean for lack of anything to
    check --, and the what-ifs alone have examined pods."""
    pods, admitting = sum(emulated[n]["checked"][1] for n in FLAT), sum(emulated[n]["admitting"] for n in FLAT)
    print(pods, admitting, sum(emulated[n]["checked"][2] for n in FLAT))
    assert pods > 0 and admitting > 0, (pods, admitting)
    assert sum(emulated[n]["checked"][1] for n in WHATIFS) > 0


@pytest.mark.parametrize("name", DERIVED)
def test_a_derived_whatif_counts_what_the_same_whatif_flattened_counts(emulated, name):
    """The batch form over what-ifs derived on the device -- the snapshot's classes, the removed nodes skipped, the results where they lie -- examines as many pods and
    pairs, as many of them admitting, as the reference does over the same what-if flattened."""
    d, p = emulated[name], emulated[name.replace("_derived", "")]
    assert (d["checked"], d["admitting"], d["skipped"], d["n_new"], d["n_placed"]) == (p["checked"], p["admitting"], p["skipped"], p["n_new"], p["n_placed"]), (d, p)


@pytest.mark.parametrize("i", range(len(FC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    """tests/audit_firstfit_cases.py: each edit through the claimed form raises exactly the reference's flags, the tampered pod's bit among them."""
    name, ok = emulated["tamper"][i]
    assert name == FC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(FC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == FC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
PLAIN, ZONE2, TEAM, NO_TEAM, PORTS, VOLUMES, NAMED, OWNER, HUGE = range(9)
E0, E1, E2, N0, N1, N2, N3 = range(7)
EX, NW, TM, SQ = FR.BITS["FIT_EXISTING"], FR.BITS["FIT_NEW"], FR.BITS["FIT_TEMPLATE"], FR.BITS["SEQ"]


def _tiny():
    """Two keys -- 0 the zone (well known, values 0 1 2), 1 `team` (a custom label, values 0 1) --, one resource, two types (4 000 and 8 000 units), three templates
    (0 limited | 1 without limits | 2 without limits, labelled team In {0}), three existing nodes with 1 000 units to spare (e0 in zone 0, e1 in zone 1, e2 without a
    label) and four new nodes (n0: template 1, no requirement | n1: template 1, ended with team In {0} | n2: template 2, team In {0} | n3: template 1, ended with team
    DoesNotExist).  Classes: 0 plain, 100 units | 1 zone In {2} | 2 team In {0} | 3 team DoesNotExist | 4 a host port | 5 a volume | 6 hostname In [e1] | 7 owns a
    topology group | 8 huge: 2 000 units, which no existing node holds.  Six pods, all plain until a case says otherwise, on e0 in commit order 0 .. 5."""
    u32, i32 = (lambda *x: np.array(x, dtype=np.uint32)), (lambda *x: np.array(x, dtype=np.int32))
    C, Pn, K = 9, 6, 2
    off = lambda ns: np.cumsum([0] + list(ns)).astype(np.uint32)
    p = {"P": Pn, "C": C, "M": 3, "E": 3, "K": K, "R": 1, "T": 2, "S": 1, "SC": 1, "wellknown_mask": 1, "key_zone": 0, "key_ct": -1, "n_ct": 0,
         "key_nvalues": u32(3, 2), "value_int": np.full(K * 64, A.NOT_INT, dtype=np.int32),
         "pod_stage_off": np.arange(Pn + 1, dtype=np.uint32), "stage_cls": np.zeros(Pn, dtype=np.uint32),
         "cls_own_off": off([1 if c == OWNER else 0 for c in range(C)]), "cls_isel_off": off([0] * C), "cls_port_off": off([1 if c == PORTS else 0 for c in range(C)]),
         "cls_vol_off": off([1 if c == VOLUMES else 0 for c in range(C)]), "cls_hn_off": off([1 if c == NAMED else 0 for c in range(C)]), "hn_list": u32(E1),
         "cls_hn_mode": np.array([1 if c == NAMED else 0 for c in range(C)], dtype=np.uint8),
         "cls_requests": np.array([2000 if c == HUGE else 100 for c in range(C)], dtype=np.int64), "cls_requests_present": np.ones(C, dtype=np.uint32),
         "cls_tolerated": np.zeros(C, dtype=np.uint64), "en_taints": np.zeros(3, dtype=np.uint64), "tmpl_taints": np.zeros(3, dtype=np.uint64),
         "en_requests": np.zeros(3, dtype=np.int64), "en_requests_present": np.ones(3, dtype=np.uint32), "en_avail": np.full(3, 1000, dtype=np.int64),
         "its_fail": np.zeros(1, dtype=np.uint8), "its_inter": np.zeros(1, dtype=np.uint16), "its_types": np.array([3], dtype=np.uint64),
         "it_present": u32(0, 0), "it_complement": u32(0, 0), "it_mask": np.zeros(K * 2, dtype=np.uint64), "it_alloc": np.array([4000, 8000], dtype=np.int64),
         "it_offer": np.array([1, 1], dtype=np.uint64), "tmpl_limit_present": u32(1, FR.UNLIMITED, FR.UNLIMITED), "tmpl_daemon": np.zeros(3, dtype=np.int64),
         "tmpl_daemon_present": np.zeros(3, dtype=np.uint32), "tmpl_types": np.array([3, 3, 3], dtype=np.uint64)}
    fams = {"tmpl": ([0, 0, 2], [[0, 0], [0, 0], [0, 1]]), "en": ([1, 1, 0], [[1, 0], [2, 0], [0, 0]]),
            "cls": ([2 if c in (TEAM, NO_TEAM) else 1 if c == ZONE2 else 0 for c in range(C)], [[4 if c == ZONE2 else 0, 1 if c == TEAM else 0] for c in range(C)])}
    for fam, (present, mask) in fams.items():
        n = len(present)
        p.update({fam + ".present": np.array(present, dtype=np.uint32), fam + ".complement": np.zeros(n, dtype=np.uint32), fam + ".mask": np.array(mask, dtype=np.uint64).reshape(-1),
                  fam + ".gt": np.full(n * K, A.NOGT, dtype=np.int32), fam + ".lt": np.full(n * K, A.NOLT, dtype=np.int32), fam + ".it_state": np.zeros(n, dtype=np.int32)})
    r = {"n_existing": 3, "n_new": 4, "pod_node": np.zeros(Pn, dtype=np.int32), "pod_stage": np.zeros(Pn, dtype=np.int32), "unscheduled": i32(), "node_tmpl": i32(1, 1, 2, 1),
         "node_present": u32(0, 2, 2, 2), "node_complement": u32(0, 0, 0, 0), "node_mask": np.array([[0, 0], [0, 1], [0, 1], [0, 0]], dtype=np.uint64),
         "node_gt": np.full((4, K), A.NOGT, dtype=np.int32), "node_lt": np.full((4, K), A.NOLT, dtype=np.int32), "node_types": np.array([3, 3, 3, 3], dtype=np.uint64),
         "node_requests_present": np.ones(4, dtype=np.uint32), "node_it_state": np.zeros(4, dtype=np.int32)}
    return p, r, np.arange(Pn, dtype=np.int32)


def _unit(name):
    """(problem, result, commit numbers, {pod: bits}, pods examined, (class, node) pairs evaluated)"""
    p, r, s = _tiny()
    cls, node = p["stage_cls"], r["pod_node"]
    EXISTING, NEW, TEMPLATES = 3, 4, 2      # what one class is evaluated against: every existing node it is labelled for, the new nodes, the unlimited templates
    want, pods, pairs = {}, 6, EXISTING + NEW + TEMPLATES      # (the plain class names no key: e2 is examined for it too)
    if name == "clean":
        pass
    elif name == "a pod on a later existing node while an earlier one has room":
        node[3] = E1; want = {3: EX}
    elif name == "an unlabelled key on an existing node: the pair is not examined":
        cls[0] = ZONE2; node[0] = N0; s[:] = [0, 1, 2, 3, 4, 5]      # e0 and e1 are in other zones; e2, Compatible with any zone, is not asked
        pairs += 2 + NEW + TEMPLATES
    elif name == "a class with ports is skipped":
        cls[3] = PORTS; node[3] = E1; pods = 5
    elif name == "a class owning a topology group is skipped":
        cls[3] = OWNER; node[3] = E1; pods = 5
    elif name == "a class with volumes is not examined against existing nodes":
        cls[3] = VOLUMES; node[3] = E1; pairs += NEW + TEMPLATES
    elif name == "a class with volumes is examined against new nodes and templates":
        cls[3] = VOLUMES; node[3] = -1; s[:] = [0, 1, 2, -1, 3, 4]; r["unscheduled"] = np.array([3], dtype=np.int32); want = {3: TM}; pairs += NEW + TEMPLATES
    elif name == "hostname In [e] never admits a new node or a template":
        cls[3] = NAMED; node[3] = -1; s[:] = [0, 1, 2, -1, 3, 4]; r["unscheduled"] = np.array([3], dtype=np.int32); want = {3: EX}; pairs += EXISTING + NEW + TEMPLATES
    elif name == "a limited template is never first_m, and a pod's own node with room does not flag its opener":
        cls[0] = HUGE; node[0] = N0; pairs += EXISTING + NEW + TEMPLATES      # template 0 would take it, and is limited; n0 itself would take another
    elif name == "an opener on the heavier of two templates that admit":
        cls[0] = HUGE; node[0] = N2; want = {0: TM}; pairs += EXISTING + NEW + TEMPLATES
    elif name == "a later pod added a custom key the template lacks: not admitted":
        cls[0] = HUGE; node[0] = N1; cls[1] = TEAM; node[1] = N1; cls[2] = TEAM; node[2] = N2      # pod 2 opened n2 while n1, final team In {0}, has room -- but n1's template never had the key
        pairs += EXISTING + NEW + TEMPLATES + NEW + TEMPLATES
    elif name == "the same node on a template that has the key: admitted":
        cls[0] = HUGE; node[0] = N1; cls[1] = TEAM; node[1] = N1; cls[2] = TEAM; node[2] = N2; r["node_tmpl"][1] = 2; want = {0: TM, 2: NW}
        pairs += EXISTING + NEW + TEMPLATES + NEW + TEMPLATES
    elif name == "node final DoesNotExist against class DoesNotExist: not admitted":
        cls[0] = HUGE; node[0] = N3; cls[1] = NO_TEAM; node[1] = N0      # pod 1 opened n0 while n3, final team DoesNotExist, has room: only the exception would let it in
        pairs += EXISTING + NEW + TEMPLATES + NEW + TEMPLATES
    elif name == "the same node without the key: admitted":
        cls[0] = HUGE; node[0] = N3; cls[1] = NO_TEAM; node[1] = N0; r["node_present"][3] = 0; want = {1: NW}
        pairs += EXISTING + NEW + TEMPLATES + NEW + TEMPLATES
    elif name == "a removed what-if node with room is not counted":
        p["removed"] = [E0]; node[:] = E1; pairs -= 1
    elif name == "the same node, not removed":
        node[:] = E1; want = {i: EX for i in range(6)}
    elif name == "a non-opener on a new node while an older new node admits":
        cls[0] = cls[1] = cls[2] = HUGE; node[0] = N0; node[1] = node[2] = N1; want = {1: NW}; pairs += EXISTING + NEW + TEMPLATES      # pod 1 opened n1 while n0 had room; pod 2 joined it
    elif name == "two pods with one commit number fail SEQ and are not examined":
        node[3] = node[4] = E1; s[4] = s[3]; want = {3: SQ, 4: SQ}; pods = 4
    else:
        raise KeyError(name)
    # the new nodes' requests: what the pods on them ask for (no daemon overhead here)
    r["node_requests"] = np.array([sum(int(p["cls_requests"][cls[q]]) for q in range(6) if node[q] == 3 + j) for j in range(4)], dtype=np.int64)
    return p, r, s, want, pods, pairs


UNIT = ["clean", "a pod on a later existing node while an earlier one has room", "an unlabelled key on an existing node: the pair is not examined", "a class with ports is skipped",
        "a class owning a topology group is skipped", "a class with volumes is not examined against existing nodes", "a class with volumes is examined against new nodes and templates",
        "hostname In [e] never admits a new node or a template", "a limited template is never first_m, and a pod's own node with room does not flag its opener",
        "an opener on the heavier of two templates that admit", "a later pod added a custom key the template lacks: not admitted", "the same node on a template that has the key: admitted",
        "node final DoesNotExist against class DoesNotExist: not admitted", "the same node without the key: admitted", "a removed what-if node with room is not counted",
        "the same node, not removed", "a non-opener on a new node while an older new node admits", "two pods with one commit number fail SEQ and are not examined"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, want, pods, pairs = _unit(name)
    flags, checked, admitting, skipped = FR.audit(p, r, s)
    assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == want
    assert checked[0] == int((r["pod_node"] >= 0).sum()) and checked[1] == pods and skipped == 6 - pods, (checked, skipped)
    assert checked[2] == pairs and 0 < admitting <= pairs, (checked, admitting)


def test_both_directions_have_unit_cases():
    flagged = [n for n in UNIT if any(b & FC.FIT for b in _unit(n)[3].values())]
    assert len(flagged) >= 7 and len(UNIT) - len(flagged) >= 9
    assert {b for n in UNIT for b in _unit(n)[3].values()} >= {EX, NW, TM, SQ}
