"""(CPU) The audit's sixth pass -- first-fit order for the pods under hostname anti-affinity and unfiltered hostname spread (include/ksolve.h ks_audit_hostfit_dev,
KS_AUDIT_POD_HFIT_*) -- validated where a correct result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_hostfit_ref.py) over every result the fourth pass's gate audits (tests/test_audit_firstfit.py: the
     emulator's committed cases through both pack kernels -- hostname_herd() and rr_problem(9013) among them --, the pack cases, the flattened what-ifs, the wide and
     the topology snapshot's what-ifs) raises NO flag; a rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source
     (karpenter_core_amd/csrc/ks_audit_hostfit.inc) is compiled into the emulator build and runs beside the reference: the two agree bit for bit, every counter
     included.  The gate is not vacuous, and on rr_problem(9013) -- where the fourth pass examines no pod -- it examines pod 810;
  b) the historical case on rr_problem(9013)'s correct result, the tamper matrix, the claimed results with indices out of range and the kernels' other paths
     (tests/audit_hostfit_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause of the rule, silent, and its counterpart that flags.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import numpy as np
import pytest

import audit_firstfit_cases as FC
import audit_harness as H
import audit_hostfit_cases as HC
import audit_hostfit_ref as HR
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
import audit_hostfit_ref as HR, audit_hostfit_cases as HC
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR, test_whatif_derived as WD
out = {}
def audited(name, f):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev, flags = HC.compare(S, f)
        out[name] = dict(HC.summary(dev), device_agrees=True)
    except AssertionError as e:
        out[name] = {"error": "device and reference differ: " + str(e)[:300]}
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
rr_cases, pack_cases = json.loads(sys.argv[1])
def problem(kind, args):
    return R.rr_problem(args["seed"]) if kind == "rr" else T.mid_problem_wide(args["seed"]) if kind == "wide" else (getattr(W, kind)(**args) if kind != "mid" else T.mid_problem(args["seed"]))
for name, kind, args in rr_cases:
    f = S.FlatProblem(problem(kind, args)); f.solve(decode=False); audited("rr/" + name, f)
    if name == "rr_9013":
        out["fourth_on_rr_9013"] = f.audit_firstfit()["checked"]["PODS"]
        out["historical"] = HC.historical_case(S, f)
    f.close()
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
    for i, d in enumerate(S.audit_hostfit_batch(derived)):
        out[tag + "_derived/%%d" %% i] = dict(HC.summary(d), device_agrees=True)
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
both_forms("wide_whatifs", S.ParsedProblem(snap), pod_node, E.WIDE_SETS)
its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
both_forms("topology_whatifs", S.ParsedProblem(snap), pod_node, json.loads(sys.argv[2]))
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in HC.run_tamper_matrix(S)]
out["range"] = [[n, ok if ok is True else str(ok)] for n, ok in HC.run_range_cases(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)[:600]] for n, ok in HC.run_shapes(S)]
out["clauses"] = [[n, ok if ok is True else str(ok)[:600]] for n, ok in HC.run_clauses(S)]
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
    """Over the committed cases the rule examined pods, evaluated count tests and found (class, node) pairs that admit; hostname_herd() is among the cases; and on
    rr_problem(9013) it examines pods where the fourth pass examines none."""
    pods, tests, admitting = (sum(emulated[n]["checked"][1] for n in FLAT), sum(emulated[n]["checked"][3] for n in FLAT), sum(emulated[n]["admitting"] for n in FLAT))
    print(pods, sum(emulated[n]["checked"][2] for n in FLAT), tests, admitting)
    assert pods > 0 and tests > 0 and admitting > 0, (pods, tests, admitting)
    assert emulated["rr/herd_600"]["checked"][1] > 0 and emulated["no_rr/herd_600"]["checked"][1] > 0
    assert emulated["rr/rr_9013"]["checked"][1] > 0 and emulated["fourth_on_rr_9013"] == 0, (emulated["rr/rr_9013"], emulated["fourth_on_rr_9013"])


def test_the_historical_case_pod_810_claimed_as_the_opener_of_an_added_node(emulated):
    """The shape of the bug the randomised net once caught in ks_pack_rr (rr family seed 9013): pod 810 given a machine of its own while the node it belongs on, opened
    earlier, has room.  In the correct result pod 810 joined a new node it did not open, so the edit is made on pod 810 itself; the pass examines it and raises HFIT_NEW."""
    h = emulated["historical"]
    print(h)
    assert h["pod_810_examined"] is True, h
    assert h["ok"] is True, h
    assert h["pod"] == HC.HISTORICAL_POD and not h["pod_810_opened_it"] and h["flags"] == HC.B["HFIT_NEW"], h
    assert h["first_pass"]["pods"] == {}, h      # (the first pass sees at most that the old node, with its requests given back, could now list more types)


@pytest.mark.parametrize("name", DERIVED)
def test_a_derived_whatif_counts_what_the_same_whatif_flattened_counts(emulated, name):
    d, p = emulated[name], emulated[name.replace("_derived", "")]
    assert (d["checked"], d["admitting"], d["skipped"], d["n_new"], d["n_placed"], d["groups"][0]) == (p["checked"], p["admitting"], p["skipped"], p["n_new"], p["n_placed"], p["groups"][0]), (d, p)


@pytest.mark.parametrize("i", range(len(HC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    name, ok = emulated["tamper"][i]
    assert name == HC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(HC.RANGE_NAMES)))
def test_claimed_indices_out_of_range_on_the_emulator(emulated, i):
    """Flags or skips, as the reference -- which never reads past a table -- says; the same cases go to the GPU only in tests/test_audit_hostfit_gpu.py, after these."""
    name, ok = emulated["range"][i]
    assert name == HC.RANGE_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(HC.CLAUSE_NAMES)))
def test_the_clauses_of_the_new_node_predicate_on_the_emulator(emulated, i):
    """tests/audit_hostfit_cases.py run_clauses: the Fits pair and the taint pair of tests/audit_firstfit_cases.py through this pass's kernels."""
    name, ok = emulated["clauses"][i]
    assert name == HC.CLAUSE_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(HC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == HC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
PLAIN, PORTS, OWNER = FC.PLAIN, FC.PORTS, FC.OWNER
E0, E1, N0, N2 = FC.E0, FC.E1, FC.N0, FC.N2
EX, NW, TM = HR.BITS["HFIT_EXISTING"], HR.BITS["HFIT_NEW"], HR.BITS["HFIT_TEMPLATE"]
ANTI, SPREAD, ZONAL, AFFINITY, FILTERED, INACTIVE = range(6)      # the groups: 0 hostname anti-affinity | 1 hostname spread, maxSkew 1 | 2 spread over the zone | 3 hostname affinity | 4 hostname spread under a node filter | 5 a hostname anti-affinity group created later
SELF = 1 << 31


def _hand(name):
    """tests/audit_firstfit_cases.py's hand-made problem -- three existing nodes with 1 000 units to spare, four new nodes, template 0 limited, six pods of 100 units on
    e0 -- with six topology groups.  Pod 3 is the subject: of class OWNER, constrained by the groups the case names, placed on e1 although e0 has room for its
    requests -- flagged HFIT_EXISTING unless a clause of the rule keeps e0 from admitting it.  Returns (problem, result, commit numbers, {pod: bits}, pods examined)."""
    p, r, s = FC._tiny()
    C, En = p["C"], p["E"]
    u32 = lambda x: np.array(x, dtype=np.uint32)
    p.update({"G": 6, "GH": 5, "grp_key": np.array([-2, -2, 0, -2, -2, -2], dtype=np.int32), "grp_type": np.array([2, 0, 0, 1, 0, 2], dtype=np.uint8),
              "grp_active": np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8), "grp_max_skew": np.array([0, 1, 1, 0, 1, 0], dtype=np.int32), "grp_count": np.zeros(6 * 64, dtype=np.int32),
              "grp_hslot": np.array([0, 1, -1, 2, 3, 4], dtype=np.int32), "grph_count": np.zeros(5 * En, dtype=np.int32),
              "grp_filter_off": u32([0, 0, 0, 0, 0, 1, 1]), "flt.present": u32([1]), "flt.it_state": np.array([0], dtype=np.int32)})
    own, sel, want, pods = {}, {}, {}, 1
    cls, node = p["stage_cls"], r["pod_node"]
    cls[3], node[3] = OWNER, E1
    init = lambda g, e, v: p["grph_count"].__setitem__(int(p["grp_hslot"][g]) * En + e, v)
    if name == "anti-affinity: e0 with a count of 0 admits":
        own[OWNER] = [ANTI]; want = {3: EX}
    elif name == "anti-affinity: a node with a count of 1":
        own[OWNER] = [ANTI]; init(ANTI, E0, 1)
    elif name == "anti-affinity: the count comes from the pods the result puts there":
        own[OWNER] = [ANTI]; sel[PLAIN] = [ANTI]
    elif name == "spread: count + self == maxSkew admits":
        own[OWNER] = [SPREAD]; init(SPREAD, E0, 1); want = {3: EX}
    elif name == "spread: count + self == maxSkew + 1":
        own[OWNER] = [SPREAD | SELF]; init(SPREAD, E0, 1)
    elif name == "init == -1: the hostname is not registered":
        own[OWNER] = [ANTI]; init(ANTI, E0, -1)
    elif name == "spread: init == -1":
        own[OWNER] = [SPREAD]; init(SPREAD, E0, -1)
    elif name.startswith("an ineligible group beside an eligible one: "):
        own[OWNER] = [ANTI, {"zonal spread": ZONAL, "hostname affinity": AFFINITY, "filtered hostname spread": FILTERED, "an inactive group": INACTIVE}[name.split(": ")[1]]]; pods = 0
    elif name == "a class with host ports":
        cls[3] = PORTS; own[PORTS] = [ANTI]; pods = 0
    elif name == "a class with empty lists":
        pods = 0
    elif name == "a limited template":
        own[OWNER] = [ANTI]; p["cls_requests"][OWNER] = 2000; node[3] = N0      # template 0 would take it on a fresh machine, and is limited; n0 is of template 1
    elif name == "the same opener on the later of two templates without limits":
        own[OWNER] = [ANTI]; p["cls_requests"][OWNER] = 2000; node[3] = N2; want = {3: TM}
    else:
        raise KeyError(name)
    off = lambda d: np.cumsum([0] + [len(d.get(c, [])) for c in range(C)]).astype(np.uint32)
    flat = lambda d: u32([x for c in range(C) for x in d.get(c, [])])
    p.update({"cls_own_off": off(own), "own_list": flat(own), "cls_sel_off": off(sel), "sel_list": flat(sel), "cls_isel_off": off({}), "isel_list": u32([]), "cls_iown_off": off({}), "iown_list": u32([])})
    r["node_requests"] = np.array([sum(int(p["cls_requests"][cls[q]]) for q in range(6) if node[q] == 3 + j) for j in range(4)], dtype=np.int64)
    return p, r, s, want, pods


UNIT = ["anti-affinity: e0 with a count of 0 admits", "anti-affinity: a node with a count of 1", "anti-affinity: the count comes from the pods the result puts there",
        "spread: count + self == maxSkew admits", "spread: count + self == maxSkew + 1", "init == -1: the hostname is not registered", "spread: init == -1",
        "an ineligible group beside an eligible one: zonal spread", "an ineligible group beside an eligible one: hostname affinity",
        "an ineligible group beside an eligible one: filtered hostname spread", "an ineligible group beside an eligible one: an inactive group", "a class with host ports",
        "a class with empty lists", "a limited template", "the same opener on the later of two templates without limits"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, want, pods = _hand(name)
    flags, checked, admitting, skipped, eligible, skipped_groups = HR.audit(p, r, s)
    assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == want
    assert checked[0] == 6 and checked[1] == pods and skipped == 6 - pods, (checked, skipped)
    assert (eligible, skipped_groups) == (2, 4)
    assert (checked[2] > 0 and checked[3] >= checked[2] and admitting > 0) if pods else (checked[2] == checked[3] == admitting == 0), (checked, admitting)


def test_the_silent_clauses_and_their_counterparts_are_both_there():
    flagged = [n for n in UNIT if _hand(n)[3]]
    assert len(flagged) == 3 and len(UNIT) - len(flagged) == 12
