"""(CPU) The audit's eighth pass -- the failure reasons, pod_reason's nibbles against what a fresh node of every template answers the pod's class (include/ksolve.h
ks_audit_reasons_dev, KS_AUDIT_POD_REASON_*) -- validated where a correct result is known, before any GPU run:
  a) soundness: the reference pass (tests/audit_reasons_ref.py) raises NO flag over every result the lane-fibre emulator returns for its committed cases -- the set
     tests/test_audit_firstfit.py audits, results proven equal to the oracle's in tests/test_rr_emulated.py, through both pack kernels, the what-ifs flattened and
     derived -- nor over tests/audit_reasons_cases.py's family of problems in which pods really stay unscheduled, each proven equal to the oracle's here first, the
     REASONS line included.  A rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source
     (karpenter_core_amd/csrc/ks_audit_reasons.inc) is compiled into the emulator build and runs beside the reference: the two agree bit for bit, counters included;
  b) exactness: for every (pod, template) the reference decides exactly, its value IS the oracle's nibble -- see test_exactness_and_non_vacuity;
  c) the tamper matrix (every edit touches pod_reason alone; all seven earlier passes and the gate stay silent) and the kernels' other paths, on the emulator,
     through both pack kernels;
  d) unit cases of the reference alone on a hand-made problem: one per clause and per exclusion.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py).

Non-vacuity, as measured over FLAT (the committed cases and the family; `python -m pytest tests/test_audit_reasons.py -k vacuity -s` prints them): 2 098 unscheduled
pods examined, 1 646 nibbles decided exactly (2: 562, 4: 341, 7: 743 -- every one equal to the nibble of the oracle-proven result), 536 bounded to a set (5: 108,
6: 1, 7: 427), 2 622 not examined (KS_WHY_LIMITS on a limited template).  The family alone: 328 pods, 886 exact (2: 396, 4: 242, 7: 248), 344 bounded (5: 106,
7: 238), 184 not examined."""
import numpy as np
import pytest

import audit_firstfit_cases as FC
import audit_harness as H
import audit_reasons_cases as RC
import audit_reasons_ref as RR
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
from oracle import oracle_py as O
import audit_reasons_cases as RC, audit_reasons_ref as RR
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR, test_whatif_derived as WD
out = {}
def audited(name, f, more=None):
    # the reference pass's findings (must be none), what it decided beside what the result carries, and whether the emulated device pass says the same
    try:
        dev, ref = RC.compare(S, f)
        out[name] = dict(RC.tally(dev, ref, f.result_arrays(), RR.problem_arrays(S, f)), device_agrees=True, **(more or {}))
    except AssertionError as e:
        out[name] = {"error": "device and reference differ: " + str(e)[:300]}
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
rr_cases, pack_cases, family = json.loads(sys.argv[1])
def problem(kind, args):
    return R.rr_problem(args["seed"]) if kind == "rr" else T.mid_problem_wide(args["seed"]) if kind == "wide" else (getattr(W, kind)(**args) if kind != "mid" else T.mid_problem(args["seed"]))
for name, kind, args in rr_cases:
    f = S.FlatProblem(problem(kind, args)); f.solve(decode=False); audited("rr/" + name, f); f.close()
    f = S.FlatProblem(problem(kind, args), flags=S.KS_FLAG_NO_RR); f.solve(decode=False); audited("no_rr/" + name, f); f.close()
for name, kind, args, no_rr in pack_cases:
    f = S.FlatProblem(E._problem(kind, args), flags=S.KS_FLAG_NO_RR if no_rr else 0); f.solve(decode=False); audited("pack/" + name, f); f.close()
for name, args in family:      # every member proven equal to the oracle's first -- the REASONS line included --, through both pack kernels
    want = O.solve(RC.stay_problem(**args))
    for tag, flags in (("family_rr/", 0), ("family_no_rr/", S.KS_FLAG_NO_RR)):
        f = S.FlatProblem(RC.stay_problem(**args), flags=flags); f.solve(decode=False)
        got = f.result()
        audited(tag + name, f, {"oracle": got.canonical() == want.canonical() and got.reasons == want.reasons and len(want.reasons) == len(want.unscheduled) > 0}); f.close()
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
    for i, d in enumerate(S.audit_reasons_batch(derived)):
        out[tag + "_derived/%%d" %% i] = dict(RC.summary(d), device_agrees=True)
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
both_forms("wide_whatifs", S.ParsedProblem(snap), pod_node, E.WIDE_SETS)
its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
both_forms("topology_whatifs", S.ParsedProblem(snap), pod_node, json.loads(sys.argv[2]))
for tag, flags in (("rr", 0), ("no_rr", S.KS_FLAG_NO_RR)):
    out["tamper/" + tag] = [[n, ok if ok is True else str(ok)] for n, ok in RC.run_tamper_matrix(S, flags)]
    out["shapes/" + tag] = [[n, ok if ok is True else str(ok)] for n, ok in RC.run_shapes(S, flags)]
print("RESULT " + json.dumps(out))
"""

TOPOLOGY_SETS = H.WHATIF_SETS
WHATIFS, COMMITTED, DERIVED = H.gate_names()
FAMILY = [tag + name for name, _ in RC.FAMILY for tag in ("family_rr/", "family_no_rr/")]
FLAT = COMMITTED + FAMILY
NAMES = FLAT + DERIVED
KERNELS = ("rr", "no_rr")


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [E.CASES, E.PACK_CASES, RC.FAMILY], TOPOLOGY_SETS)


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got.get("oracle", True) is True, "the family's result is not the oracle's"
    assert got["pods"] == {}, got["pods"]
    assert got["device_agrees"], got


def test_exactness_and_non_vacuity(emulated):
    """Summed over the committed cases and the family.  Exactness: every nibble the reference decides exactly equals the nibble the oracle-proven result carries --
    not one disagrees.  Non-vacuity: pods examined, exact, bounded and unexamined nibbles are each non-zero; among the exact ones KS_WHY_TAINTS, _REQUIREMENTS and
    _NO_INSTANCE_TYPE are each seen (KS_WHY_NONE cannot be: an unscheduled pod never carries it); among the bounded ones TOPOLOGY and NO_INSTANCE_TYPE; among the
    unexamined ones LIMITS.  The family alone reaches all of this."""
    def sums(names):
        exact, bounded, unexamined = {}, {}, {}
        for n in names:
            for k, (yes, no) in emulated[n]["exact"].items():
                e = exact.setdefault(int(k), [0, 0]); e[0] += yes; e[1] += no
            for src, dst in ((emulated[n]["bounded"], bounded), (emulated[n]["unexamined"], unexamined)):
                for k, v in src.items():
                    dst[int(k)] = dst.get(int(k), 0) + v
        return {"pods": sum(emulated[n]["checked"][0] for n in names), "exact": sum(emulated[n]["checked"][1] for n in names), "bounded": sum(emulated[n]["checked"][2] for n in names),
                "unexamined": sum(emulated[n]["checked"][3] for n in names), "exact by value [agree, disagree]": exact, "bounded by value": bounded, "unexamined by value": unexamined}
    for names in (FLAT, FAMILY):
        got = sums(names)
        print("the family alone:" if names is FAMILY else "committed cases and family:", got)
        W = RR.WHY
        assert all(got[k] > 0 for k in ("pods", "exact", "bounded", "unexamined")), got
        exact = got["exact by value [agree, disagree]"]
        assert all(no == 0 for _, no in exact.values()), exact
        assert sum(yes for yes, _ in exact.values()) == got["exact"]
        assert all(exact.get(v, [0, 0])[0] > 0 for v in (W["TAINTS"], W["REQUIREMENTS"], W["NO_INSTANCE_TYPE"])) and W["NONE"] not in exact, exact
        assert got["bounded by value"].get(W["TOPOLOGY"], 0) > 0 and got["bounded by value"].get(W["NO_INSTANCE_TYPE"], 0) > 0 and set(got["bounded by value"]) <= {5, 6, 7}, got["bounded by value"]
        assert set(got["unexamined by value"]) == {W["LIMITS"]} and sum(got["unexamined by value"].values()) == got["unexamined"], got["unexamined by value"]


def test_a_word_carries_different_nibbles_and_the_ninth_template_has_none(emulated):
    """The family's members have one, two, four, eight and nine templates of mixed kinds; the per-member identity EXACT + BOUNDED + UNEXAMINED == min(M, 8) * PODS holds,
    and pairs == min(M, 8) * used classes: a ninth template is evaluated for no class."""
    seen = set()
    for name, args in RC.FAMILY:
        M = len(args["kinds"])
        seen.add(M)
        for tag in ("family_rr/", "family_no_rr/"):
            g = emulated[tag + name]
            assert sum(g["checked"][1:]) == min(M, 8) * g["checked"][0] and g["pairs"] == min(M, 8) * g["used_classes"] and g["n_unscheduled"] == g["checked"][0], g
    assert seen >= {1, 2, 8, 9}


@pytest.mark.parametrize("name", DERIVED)
def test_a_derived_whatif_counts_what_the_same_whatif_flattened_counts(emulated, name):
    d, p = emulated[name], emulated[name.replace("_derived", "")]
    keys = ("pods", "checked", "skipped_pods", "n_unscheduled", "used_classes", "pairs", "n_new", "n_placed")
    assert [d[k] for k in keys] == [p[k] for k in keys], (d, p)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("i", range(len(RC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i, kernel):
    """tests/audit_reasons_cases.py: each edit of pod_reason through the claimed form raises exactly its bit on exactly its pod, device and reference alike, and all
    seven earlier passes -- the gate's six in one call, the seventh beside it -- are silent on it."""
    name, ok = emulated["tamper/" + kernel][i]
    assert name == RC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


def test_every_bit_has_an_edit():
    res = {"pod_node": np.array([0, -1, -1, -1], dtype=np.int32), "pod_reason": np.array([0, 0x7727, 0x7427, 0x5525], dtype=np.uint32)}
    wants = RC.tampers(res, ["fill-0", "giant-0", "z2giant-0", "za-0"])
    bits = 0
    for _, _, want in wants:
        for b in want.values():
            bits |= b
    assert bits == sum(RR.BITS.values()) and all(len(w) == 1 for _, _, w in wants)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("i", range(len(RC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i, kernel):
    name, ok = emulated["shapes/" + kernel][i]
    assert name == RC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
PLAIN, ZONE2, TEAM, NO_TEAM, PORTS, VOLUMES, NAMED, OWNER, HUGE = FC.CLASSES
E0 = FC.NODES[0]
PL, MI, SH, ST = (RR.BITS[k] for k in ("REASON_PLACED", "REASON_MISSING", "REASON_SHAPE", "REASON_STATIC"))
TAINT_ALL, TAINT_2 = (1, 1, 1), (0, 0, 1)

# name: (the class of pod 0, which is claimed unscheduled; the templates' taints; the nibbles of its word from template 0 on; its flags; checked).  The problem is
# tests/audit_firstfit_cases.py's: template 0 limited, 1 and 2 without limits, 2 labelled team In {0}; HUGE here asks for more than any type holds.
UNITS = {
    "a class every template would take: only the limited one may say NO_INSTANCE_TYPE": (PLAIN, None, [7, 7, 7], ST, [1, 3, 0, 0]),
    "no type holds the class": (HUGE, None, [7, 7, 7], 0, [1, 3, 0, 0]),
    "LIMITS on the limited template is allowed and not examined": (HUGE, None, [1, 7, 7], 0, [1, 2, 0, 1]),
    "LIMITS on a template without limits": (HUGE, None, [7, 1, 7], SH, [1, 3, 0, 0]),
    "a custom label two templates do not define": (TEAM, TAINT_2, [4, 4, 2], 0, [1, 3, 0, 0]),
    "the same, said as NO_INSTANCE_TYPE": (TEAM, TAINT_2, [7, 4, 2], ST, [1, 3, 0, 0]),
    "the template that defines the label takes the class": (TEAM, None, [4, 4, 4], ST, [1, 3, 0, 0]),
    "taints come before requirements": (TEAM, TAINT_ALL, [2, 2, 2], 0, [1, 3, 0, 0]),
    "requirements said where a taint refuses first": (TEAM, TAINT_ALL, [4, 4, 2], ST, [1, 3, 0, 0]),
    "DoesNotExist passes where the label is undefined and fails where it is defined": (NO_TEAM, None, [7, 0, 4], MI, [1, 3, 0, 0]),
    "DoesNotExist against the template that defines the label, the others tainted": (NO_TEAM, (1, 1, 0), [2, 2, 4], 0, [1, 3, 0, 0]),
    "a hostname selector":(NAMED, None, [4, 4, 4], 0, [1, 3, 0, 0]),
    "a class with a host port is bounded": (PORTS, None, [5, 6, 7], 0, [1, 0, 3, 0]),
    "a bounded nibble outside its set": (PORTS, None, [5, 4, 7], ST, [1, 0, 3, 0]),
    "a class that owns a group, on a tainted template": (OWNER, TAINT_2, [6, 6, 2], 0, [1, 1, 2, 0]),
    "a zeroed nibble": (HUGE, None, [7, 0, 7], MI, [1, 3, 0, 0]),
    "a nibble at m == M": (HUGE, None, [7, 7, 7, 7], SH, [1, 3, 0, 0]),
    "HOST_PORTS cannot occur": (HUGE, None, [7, 3, 7], SH, [1, 3, 0, 0]),
    "a nibble above 7": (HUGE, None, [7, 7, 12], SH, [1, 3, 0, 0]),
    "a zeroed nibble and a wrong one": (TEAM, None, [0, 7, 4], MI | ST, [1, 3, 0, 0]),
}


def _unit(name):
    cls, taints, word, want, checked = UNITS[name]
    p, r, _ = FC._tiny()
    p["cls_requests"][HUGE] = 9000
    p["stage_cls"] = np.array([cls] + [PLAIN] * 5, dtype=np.uint32)
    if taints:
        p["tmpl_taints"] = np.array(taints, dtype=np.uint64)
    r["pod_node"][0] = -1
    r["pod_reason"] = np.zeros(6, dtype=np.uint32)
    r["pod_reason"][0] = sum(v << (4 * m) for m, v in enumerate(word))
    return p, r, ({0: want} if want else {}), checked


@pytest.mark.parametrize("name", list(UNITS))
def test_reference_pass_on_a_hand_made_result(name):
    p, r, want, checked = _unit(name)
    got = RR.audit(p, r)
    assert H.flagged(got["pod_flags"]) == want, (H.flagged(got["pod_flags"]), got["verdicts"])
    assert got["checked"] == checked and got["n_placed"] == 5 and got["n_unscheduled"] == 1 and got["skipped_pods"] == 0 and got["pairs"] == 3 and got["used_classes"] == 1, got


def test_reference_pass_exclusions():
    p, r, _, _ = _unit("no type holds the class")
    r["pod_reason"][1] = 7      # a placed pod with a word
    got = RR.audit(p, r)
    assert H.flagged(got["pod_flags"]) == {1: PL}
    r["pod_reason"][1] = 0
    r["pod_stage"][0] = 5       # a stage outside the chain: the pod is skipped, nothing is addressed
    got = RR.audit(p, r)
    assert not got["pod_flags"].any() and got["checked"] == [0, 0, 0, 0] and got["skipped_pods"] == 1 and got["n_unscheduled"] == 1 and got["pairs"] == 0
    r["pod_stage"][0] = 0
    p["tmpl_types"] = np.array([3, 0, 3], dtype=np.uint64)      # a template without types is not examined, whatever its nibble says
    r["pod_reason"][0] = 0x757
    got = RR.audit(p, r)
    assert not got["pod_flags"].any() and got["checked"] == [1, 2, 0, 1]
    p["removed"] = [E0]         # the pods on a node that left a what-if name no node of the result: neither placed nor unscheduled
    r["pod_reason"][1] = 7
    got = RR.audit(p, r)
    assert not got["pod_flags"].any() and got["n_placed"] == 0 and got["skipped_pods"] == 5


def test_both_directions_have_unit_cases():
    wants = [UNITS[n][3] for n in UNITS]
    assert sum(1 for w in wants if w) >= 8 and sum(1 for w in wants if not w) >= 8
    assert {ST, SH, MI, MI | ST} <= set(wants)
