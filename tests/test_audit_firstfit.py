"""(CPU) The audit's fourth pass -- first-fit order from the final state and the commit numbers (include/ksolve.h ks_audit_firstfit_dev, KS_AUDIT_POD_FIT_*) --
validated where a correct result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_firstfit_ref.py) over every result the lane-fibre emulator returns for its committed cases -- the set
     tests/test_audit_spread.py audits, results proven equal to the oracle's in tests/test_rr_emulated.py -- and over the what-ifs of tests/test_whatif_derived.py's
     decorated snapshot raises NO flag; a rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source
     (karpenter_core_amd/csrc/ks_audit_firstfit.inc) is compiled into the emulator build and runs beside the reference: the two agree bit for bit, `checked`,
     `admitting_pairs` and `skipped_pods` included.  Over the set the rule examined pods, and some (class, node) pairs admitted;
  b) the tamper matrix, the kernels' other paths and the clauses of the new-node predicate in pairs (tests/audit_firstfit_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause of the rule and per direction.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import numpy as np
import pytest

import audit_firstfit_cases as FC
import audit_firstfit_ref as FR
import audit_harness as H
import test_rr_emulated as E

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
out["clauses"] = [[n, ok if ok is True else str(ok)] for n, ok in FC.run_clauses(S)]
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


@pytest.mark.parametrize("i", range(len(FC.CLAUSE_NAMES)))
def test_the_clauses_of_the_new_node_predicate_on_the_emulator(emulated, i):
    """tests/audit_firstfit_cases.py run_clauses: per clause a pair of claimed results that differ in that clause alone -- the reference refuses the one and admits the
    other, and the kernels say what it says, counters included."""
    name, ok = emulated["clauses"][i]
    assert name == FC.CLAUSE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
PLAIN, ZONE2, TEAM, NO_TEAM, PORTS, VOLUMES, NAMED, OWNER, HUGE = FC.CLASSES
E0, E1, E2, N0, N1, N2, N3 = FC.NODES
EX, NW, TM, SQ = FR.BITS["FIT_EXISTING"], FR.BITS["FIT_NEW"], FR.BITS["FIT_TEMPLATE"], FR.BITS["SEQ"]


def _unit(name):
    """(problem, result, commit numbers, {pod: bits}, pods examined, (class, node) pairs evaluated)"""
    p, r, s = FC._tiny()
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
