"""(CPU) The audit's fifth pass -- provisioner limits from the final state and the commit numbers (include/ksolve.h ks_audit_limits_dev, KS_AUDIT_NODE_LIMIT_*,
KS_AUDIT_POD_LIMIT_TEMPLATE) -- validated where a correct result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_limits_ref.py) raises NO flag over the results the lane-fibre emulator returns for the committed cases of
     tests/test_rr_emulated.py that carry a limited template (the fuzz and the wide families, results proven equal to the oracle's there), for a small instance of the
     config #5 generator, and for a seeded family of small problems made for this pass -- one to three provisioners, limits on one or two of cpu / memory / a device
     resource, existing nodes of the limited provisioner so that its remaining resources start low or negative --, each of the latter two first proven equal to the
     oracle's here; a rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source (karpenter_core_amd/csrc/ks_audit_limits.inc) is
     compiled into the emulator build and runs beside the reference: the two agree bit for bit, every counter included;
  b) the tamper matrix, the pinned one-sidedness, a batch of what-ifs derived on the device and the kernels' other paths (tests/audit_limits_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause of the rule and per direction.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import numpy as np
import pytest

import audit_harness as H
import audit_limits_cases as LC
import audit_limits_ref as LR
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
from oracle import oracle_py
import audit_limits_ref as LR, audit_limits_cases as LC
import test_rr_emulated as E
out = {}
def audited(name, f, extra=None):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev, ref = LC.compare(S, f)
        out[name] = dict(LC.summary(dev), device_agrees=True, **(extra or {}))
    except AssertionError as e:
        out[name] = {"error": "device and reference differ: " + str(e)[:300]}
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
for name, kind, args, no_rr in json.loads(sys.argv[1]):
    f = S.FlatProblem(E._problem(kind, args), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    if (LR.problem_arrays(S, f)["tmpl_limit_present"] != LR.UNLIMITED).any():
        f.solve(decode=False); audited("pack/" + name, f)
    else:
        out["pack/" + name] = {"unlimited": True}
    f.close()
def proven(name, pr):
    f = S.FlatProblem(pr, flags=S.KS_FLAG_NO_RR)
    got = f.solve()
    same = got.canonical() == oracle_py.solve(pr).canonical()
    ra = f.result_arrays()
    why = any(((int(ra["pod_reason"][p]) >> (4 * m)) & 15) == LC.KS_WHY_LIMITS for p in ra["unscheduled"] for m in range(min(8, f.dims["M"])))
    audited(name, f, {"oracle": same, "why_limits": bool(why)})
    f.close()
proven("config5", W.config5(pods=400, sizes=3, seed=46))
for seed in LC.FAMILY_SEEDS:
    proven("family/%%d" %% seed, LC.family_problem(seed))
try:
    out["whatifs"] = LC.run_whatifs(S)
except AssertionError as e:
    out["whatifs"] = "differs: " + str(e)[:400]
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in LC.run_tamper_matrix(S)]
out["one_sided"] = [[n, ok if ok is True else str(ok)] for n, ok in LC.run_one_sided(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)] for n, ok in LC.run_shapes(S)]
print("RESULT " + json.dumps(out))
"""

PACK = [c for c in E.PACK_CASES if c[1] in ("fuzz", "wide_sparse", "wide_dense")]
FAMILY = ["family/%d" % s for s in LC.FAMILY_SEEDS]
PROVEN = ["config5"] + FAMILY


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, PACK)


@pytest.mark.parametrize("name", ["pack/" + c[0] for c in PACK] + PROVEN)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    if got.get("unlimited"):
        return      # no limited template: not this pass's subject
    assert "error" not in got, got
    assert got.get("oracle", True), "the emulator's result is not the oracle's"
    assert got["pods"] == {} and got["nodes"] == {}, got
    assert got["device_agrees"], got


def test_the_gate_is_not_vacuous(emulated):
    """The committed families carry limited templates whose nodes were examined -- the wide family's among them --, and the seeded family meets what it was tuned for
    on the CPU with the reference alone: the limit excludes a type in at least half of the seeds; exact nodes, and nodes that are not, in at least five each; an
    unscheduled pod with KS_WHY_LIMITS in at least five."""
    limited = [n for n in ("pack/" + c[0] for c in PACK) if not emulated[n].get("unlimited")]
    assert any(n.startswith("pack/wide_") for n in limited) and sum(emulated[n]["checked"][1] for n in limited) > 0, limited
    assert emulated["config5"]["limited_templates"] >= 1
    fam = [emulated[n] for n in FAMILY]
    print(sum(f["binding_nodes"] > 0 for f in fam), sum(f["exact_nodes"] > 0 for f in fam), sum(0 < f["exact_nodes"] < f["checked"][1] for f in fam), sum(f["why_limits"] for f in fam))
    assert len(fam) >= 40 and all(f["limited_templates"] >= 1 for f in fam)
    assert 2 * sum(f["binding_nodes"] > 0 for f in fam) >= len(fam)
    assert sum(f["exact_nodes"] > 0 for f in fam) >= 5 and sum(f["exact_nodes"] < f["checked"][1] for f in fam) >= 5
    assert sum(f["why_limits"] for f in fam) >= 5


def test_a_batch_of_derived_whatifs_over_a_limited_snapshot(emulated):
    """tests/audit_limits_cases.py run_whatifs: six what-ifs of a 24-node snapshot whose provisioner is limited to the cpu its nodes hold, derived on the device
    against flattened one by one."""
    got = emulated["whatifs"]
    assert isinstance(got, list) and len(got) == len(LC.WHATIF_SETS), got


@pytest.mark.parametrize("i", range(len(LC.TAMPER_REPORT_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    """tests/audit_limits_cases.py: each edit through the claimed form raises exactly the reference's flags, and the bits the rule names for it."""
    name, ok = emulated["tamper"][i]
    assert name == LC.TAMPER_REPORT_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(LC.ONE_SIDED_NAMES)))
def test_one_sidedness_is_pinned_on_the_emulator(emulated, i):
    name, ok = emulated["one_sided"][i]
    assert name == LC.ONE_SIDED_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(LC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == LC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
EX, MI, LT, SQ = LR.NODE_BITS["LIMIT_EXTRA"], LR.NODE_BITS["LIMIT_MISSING"], LR.POD_BITS["LIMIT_TEMPLATE"], LR.POD_BITS["SEQ"]


def _tiny():
    """No key, two resources (0 cpu, 1 a device), four types -- cpu / devices: t0 2 / 0, t1 6 / 0, t2 4 / 2, t3 8 / 4; allocatable == capacity --, three templates
    (0 limited on cpu, R0 = 10 | 1 limited on cpu and the device, R0 = 18 / 4, tainted: no class tolerates it | 2 without limits), no existing node and three new
    nodes -- n0 of template 0 {t3}, opened at commit 0 by pod 0 (class 0: 7 cpu, only t3 holds it); n1 of template 0 {t0}, opened at commit 1 by pod 1 (class 1:
    1 cpu) out of the 2 cpu that remained; n2 of template 2 {t1, t2, t3}, opened at commit 2 by pod 2 (class 2: 3 cpu) when nothing remained to template 0.  Class 3
    is class 1 owning a topology group."""
    u32, i32, i64 = (lambda *x: np.array(x, dtype=np.uint32)), (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.int64))
    C, Pn, K, R, T, M = 4, 3, 0, 2, 4, 3
    off = lambda ns: np.cumsum([0] + list(ns)).astype(np.uint32)
    p = {"P": Pn, "C": C, "M": M, "E": 0, "K": K, "R": R, "T": T, "S": 1, "SC": 1, "wellknown_mask": 0, "key_zone": -1, "key_ct": -1, "n_ct": 0,
         "key_nvalues": u32(), "value_int": np.zeros(0, dtype=np.int32),
         "pod_stage_off": np.arange(Pn + 1, dtype=np.uint32), "stage_cls": u32(0, 1, 2),
         "cls_own_off": off([0, 0, 0, 1]), "cls_isel_off": off([0] * C), "cls_port_off": off([0] * C), "cls_hn_mode": np.zeros(C, dtype=np.uint8),
         "cls_requests": i64(7000, 0, 1000, 0, 3000, 0, 1000, 0), "cls_requests_present": np.ones(C, dtype=np.uint32),
         "cls_tolerated": np.zeros(C, dtype=np.uint64), "tmpl_taints": np.array([0, 1, 0], dtype=np.uint64),
         "its_fail": np.zeros(1, dtype=np.uint8), "its_inter": np.zeros(1, dtype=np.uint16), "its_types": np.array([15], dtype=np.uint64),
         "it_present": np.zeros(T, dtype=np.uint32), "it_complement": np.zeros(T, dtype=np.uint32), "it_mask": np.zeros(0, dtype=np.uint64),
         "it_alloc": i64(2000, 6000, 4000, 8000, 0, 0, 2, 4), "it_cap": i64(2000, 6000, 4000, 8000, 0, 0, 2, 4), "it_offer": np.ones(T, dtype=np.uint64),
         "tmpl_limit_present": u32(1, 3, LR.UNLIMITED), "tmpl_remaining": i64(10000, 0, 18000, 4, 0, 0), "tmpl_daemon": np.zeros(M * R, dtype=np.int64),
         "tmpl_daemon_present": np.zeros(M, dtype=np.uint32), "tmpl_types": np.array([15, 15, 15], dtype=np.uint64)}
    for fam, n in (("tmpl", M), ("cls", C)):
        p.update({fam + ".present": np.zeros(n, dtype=np.uint32), fam + ".complement": np.zeros(n, dtype=np.uint32), fam + ".mask": np.zeros(0, dtype=np.uint64),
                  fam + ".gt": np.zeros(0, dtype=np.int32), fam + ".lt": np.zeros(0, dtype=np.int32), fam + ".it_state": np.zeros(n, dtype=np.int32)})
    r = {"n_existing": 0, "n_new": 3, "pod_node": i32(0, 1, 2), "pod_stage": np.zeros(Pn, dtype=np.int32), "unscheduled": i32(), "node_tmpl": i32(0, 0, 2),
         "node_present": np.zeros(3, dtype=np.uint32), "node_complement": np.zeros(3, dtype=np.uint32), "node_mask": np.zeros((3, 0), dtype=np.uint64),
         "node_gt": np.zeros((3, 0), dtype=np.int32), "node_lt": np.zeros((3, 0), dtype=np.int32), "node_types": np.array([8, 1, 14], dtype=np.uint64),
         "node_requests": i64(7000, 0, 1000, 0, 3000, 0), "node_requests_present": np.ones(3, dtype=np.uint32), "node_it_state": np.zeros(3, dtype=np.int32)}
    return p, r, np.arange(Pn, dtype=np.int32)


def _two_resources(p, r):
    """The tiny problem turned to template 1 (cpu 18, devices 4; template 0 tainted instead): three pods of class 1, one machine each.  n0 keeps every type and
    takes 8 / 4; n1 opens at 10 / 0 -- the DEVICE alone refuses t2 and t3 -- with {t0, t1} and takes 6 / 0; n2 opens at 4 / 0 -- the CPU alone refuses t1 -- with {t0}."""
    p["tmpl_taints"][:] = [1, 0, 0]; p["stage_cls"][:] = 1
    r["node_tmpl"][:] = 1; r["node_types"][:] = [15, 3, 1]; r["node_requests"][:] = [1000, 0, 1000, 0, 1000, 0]


def _one_opening(p, r, s, cls):
    """The tiny problem with one machine of template 0: pod 1, of class `cls`, opened n1 of template 2 at commit 1, pod 2 joined it; 2 cpu remained to template 0."""
    p["stage_cls"][1] = cls
    r["n_new"] = 2; r["pod_node"][:] = [0, 1, 1]; r["node_tmpl"][:2] = [0, 2]; r["node_types"][1] = 14; r["node_requests"][2] = 4000


def _unit(name):
    """(problem, result, commit numbers, {node: bits}, {pod: bits}, expected counters)"""
    p, r, s = _tiny()
    nodes, pods = {}, {}
    want = {"limited_templates": 2, "skipped_nodes": 0, "skipped_pods": 0, "exact_nodes": 2, "binding_nodes": 1, "checked": [3, 2, 3, 6]}
    if name == "clean":
        pass
    elif name == "an option above the upper bound":
        r["node_types"][1] = 3; nodes = {1: EX}      # t1 has 6 cpu, 2 remained
    elif name == "an option within the lower bound is absent":
        r["node_types"][1] = 0; nodes = {1: MI}      # t0 holds the pod and is within the 2 cpu that remained
    elif name == "limits = {}: limited, with no limited resource":
        p["tmpl_limit_present"][0] = 0; r["node_tmpl"][2] = 0; nodes = {1: MI}      # n1 must keep every type that holds 1 cpu, n2 every one that holds 3 -- as it does
        want.update(checked=[3, 3, 3, 6], exact_nodes=3, binding_nodes=0)
    elif name == "an unscheduled pod that the end state still admits":
        _one_opening(p, r, s, 1); r["pod_node"][1] = -1; s[:] = [0, -1, 1]; r["unscheduled"] = np.array([1], dtype=np.int32); r["node_requests"][2] = 3000
        pods = {1: LT}; want.update(checked=[2, 1, 3, 6], exact_nodes=1, binding_nodes=0)      # 2 cpu remain to template 0, and t0 holds 1 cpu
    elif name == "an unscheduled pod that nothing admits":
        _one_opening(p, r, s, 0); r["pod_node"][1] = -1; s[:] = [0, -1, 1]; r["unscheduled"] = np.array([1], dtype=np.int32); r["node_requests"][2] = 3000
        want.update(checked=[2, 1, 3, 4], exact_nodes=1, binding_nodes=0)      # a second pod of 7 cpu: nothing within 2 cpu holds it
    elif name == "an opener that passed over a limited template with room":
        _one_opening(p, r, s, 1); pods = {1: LT}; want.update(exact_nodes=1, binding_nodes=0, checked=[3, 1, 3, 6])
    elif name == "the same opener under a topology group: not examined on the pod side":
        _one_opening(p, r, s, 3); want.update(exact_nodes=1, binding_nodes=0, checked=[3, 1, 2, 4], skipped_pods=1)
    elif name == "nodes taken in opening order, not in index order":
        r["node_types"][:2] = [1, 8]; r["pod_node"][:2] = [1, 0]; r["node_requests"][:4] = [1000, 0, 7000, 0]      # n1 {t3} opened at commit 0, n0 {t0} at commit 1
    elif name == "the commit numbers exchanged: the small machine opened first":
        s[:] = [1, 0, 2]; nodes = {1: MI}; want.update(exact_nodes=1, binding_nodes=0)      # n1 {t0} opened with 10 cpu: t1, t2, t3 are missing; n0 then had between 2 and 8
    elif name == "R0 negative: every option is extra":
        p["tmpl_remaining"][0] = -3000; nodes = {0: EX, 1: EX}; want.update(exact_nodes=1, binding_nodes=2)
    elif name == "a sum that would pass INT64_MIN stays there":
        p["tmpl_remaining"][0] = -2 ** 63 + 1000; nodes = {0: EX, 1: EX}; want.update(exact_nodes=1, binding_nodes=2)
    elif name == "an unordered node voids the lower bound, not the upper":
        s[1] = s[0]; p["tmpl_remaining"][0] = 7000; r["node_types"][1] = 0; pods = {0: SQ, 1: SQ}; nodes = {0: EX}      # U = R0 = 7 for both: t3 is out; n1 without t0 is not MISSING
        want.update(checked=[3, 2, 1, 1], skipped_nodes=2, skipped_pods=2, exact_nodes=0, binding_nodes=2)
    elif name == "two limited resources, each binding on a different node":
        _two_resources(p, r); want.update(checked=[3, 3, 3, 2], exact_nodes=3, binding_nodes=2)
    elif name == "two limited resources: the cpu alone refuses an option of the last node":
        _two_resources(p, r); r["node_types"][2] = 3; nodes = {2: EX}; want.update(checked=[3, 3, 3, 2], exact_nodes=3, binding_nodes=2)
    elif name == "two limited resources: the device alone refuses an option of the second node":
        _two_resources(p, r); r["node_types"][1] = 7; nodes = {1: EX, 2: EX}      # (and n2 then opened with devices below zero)
        want.update(checked=[3, 3, 3, 2], exact_nodes=2, binding_nodes=2)
    else:
        raise KeyError(name)
    return p, r, s, nodes, pods, want


UNIT = ["clean", "an option above the upper bound", "an option within the lower bound is absent", "limits = {}: limited, with no limited resource",
        "an unscheduled pod that the end state still admits", "an unscheduled pod that nothing admits", "an opener that passed over a limited template with room",
        "the same opener under a topology group: not examined on the pod side", "nodes taken in opening order, not in index order",
        "the commit numbers exchanged: the small machine opened first", "R0 negative: every option is extra", "a sum that would pass INT64_MIN stays there",
        "an unordered node voids the lower bound, not the upper", "two limited resources, each binding on a different node",
        "two limited resources: the cpu alone refuses an option of the last node", "two limited resources: the device alone refuses an option of the second node"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, nodes, pods, want = _unit(name)
    got = LR.audit(p, r, s)
    assert {int(i): int(got["node_flags"][i]) for i in np.nonzero(got["node_flags"])[0]} == nodes
    assert {int(i): int(got["pod_flags"][i]) for i in np.nonzero(got["pod_flags"])[0]} == pods
    assert {k: (list(got[k]) if k == "checked" else got[k]) for k in want} == want


def test_both_directions_have_unit_cases():
    flagged = [n for n in UNIT if _unit(n)[3] or any(b & LT for b in _unit(n)[4].values())]
    assert len(flagged) >= 8 and len(UNIT) - len(flagged) >= 5
    assert {b for n in UNIT for b in list(_unit(n)[3].values()) + list(_unit(n)[4].values())} >= {EX, MI, LT, SQ}
