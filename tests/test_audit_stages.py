"""(CPU) The audit's seventh pass -- relaxation order from the final state (include/ksolve.h ks_audit_stages_dev, KS_AUDIT_POD_STAGE_*) -- validated where a correct
result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_stages_ref.py) raises NO flag over every result the lane-fibre emulator returns for its committed cases
     -- the set tests/test_audit_firstfit.py audits, results proven equal to the oracle's in tests/test_rr_emulated.py, through both pack kernels, the what-ifs
     flattened and derived -- nor over tests/audit_stages_cases.py's family of problems in which pods really relax, each proven equal to the oracle's here first.  A
     rule that flagged one of them would be a wrong rule, not a finding.  The kernels' own source (karpenter_core_amd/csrc/ks_audit_stages.inc) is compiled into
     the emulator build and runs beside the reference: the two agree bit for bit, counters included.  The run is not vacuous: see test_the_gate_is_not_vacuous;
  b) the tamper matrix and the kernels' other paths (tests/audit_stages_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause and per exclusion.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py).

Non-vacuity, as measured over FLAT (the committed cases and the family; `python -m pytest tests/test_audit_stages.py -k vacuous -s` prints them): 669 examined pods,
1 255 examined stages, 3 493 existing-node pairs, 561 template pairs, 160 unscheduled pods with an examined earlier stage; no pair admitted."""
import numpy as np
import pytest

import audit_firstfit_cases as FC
import audit_harness as H
import audit_stages_cases as SC
import audit_stages_ref as SR
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
from oracle import oracle_py as O
import audit_stages_cases as SC
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR, test_whatif_derived as WD
out = {}
def audited(name, f, more=None):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev, ref = SC.compare(S, f)
        out[name] = dict(SC.summary_with_reference(dev, ref), device_agrees=True, **(more or {}))
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
for name, args in family:      # every member proven equal to the oracle's first, through both pack kernels
    want = O.solve(SC.relax_problem(**args)).canonical()
    for tag, flags in (("family_rr/", 0), ("family_no_rr/", S.KS_FLAG_NO_RR)):
        f = S.FlatProblem(SC.relax_problem(**args), flags=flags); f.solve(decode=False)
        audited(tag + name, f, {"oracle": f.result().canonical() == want}); f.close()
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
    for i, d in enumerate(S.audit_stages_batch(derived)):
        out[tag + "_derived/%%d" %% i] = dict(SC.summary(d), device_agrees=True)
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
both_forms("wide_whatifs", S.ParsedProblem(snap), pod_node, E.WIDE_SETS)
its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
both_forms("topology_whatifs", S.ParsedProblem(snap), pod_node, json.loads(sys.argv[2]))
try:
    plain, derived = SC.derived_whatifs(S)
    out["relax_whatifs"] = {"plain": plain, "derived": derived}
except AssertionError as e:
    out["relax_whatifs"] = {"error": str(e)[:300]}
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in SC.run_tamper_matrix(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)] for n, ok in SC.run_shapes(S)]
print("RESULT " + json.dumps(out))
"""

TOPOLOGY_SETS = H.WHATIF_SETS
WHATIFS, COMMITTED, DERIVED = H.gate_names()
FAMILY = [tag + name for name, _ in SC.FAMILY for tag in ("family_rr/", "family_no_rr/")]
FLAT = COMMITTED + FAMILY
NAMES = FLAT + DERIVED


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [E.CASES, E.PACK_CASES, SC.FAMILY], TOPOLOGY_SETS)


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got.get("oracle", True) is True, "the family's result is not the oracle's"
    assert got["pods"] == {}, got["pods"]
    assert got["device_agrees"], got


def test_the_gate_is_not_vacuous(emulated):
    """Summed over the committed cases and the family: examined pods, examined stages, existing-node pairs, template pairs and unscheduled pods with an examined earlier
    stage are each non-zero -- the clean results above were not clean for lack of anything to check."""
    total = lambda f: sum(f(emulated[n]) for n in FLAT)
    counts = {"examined pods": total(lambda g: g["checked"][1]), "examined stages": total(lambda g: g["checked"][2]), "existing-node pairs": total(lambda g: g["pairs_existing"]),
              "template pairs": total(lambda g: g["pairs_template"]), "unscheduled pods with an examined earlier stage": total(lambda g: g["unscheduled_examined"])}
    print(counts, {"committed alone": {k: sum(emulated[n][k] if isinstance(emulated[n].get(k), int) else 0 for n in COMMITTED) for k in ("pairs_existing", "pairs_template", "unscheduled_examined")},
                   "committed examined": [sum(emulated[n]["checked"][i] for n in COMMITTED) for i in (1, 2)]})
    assert all(v > 0 for v in counts.values()), counts
    assert total(lambda g: g["admitting"]) == 0      # a pair that admitted would be a flag


@pytest.mark.parametrize("name", DERIVED)
def test_a_derived_whatif_counts_what_the_same_whatif_flattened_counts(emulated, name):
    d, p = emulated[name], emulated[name.replace("_derived", "")]
    assert (d["checked"], d["admitting"], d["skipped"], d["n_new"], d["n_placed"]) == (p["checked"], p["admitting"], p["skipped"], p["n_new"], p["n_placed"]), (d, p)


def test_derived_whatifs_whose_pods_relax(emulated):
    """tests/audit_stages_cases.py's snapshot, whose bound pods carry preferences nothing satisfies: flattened and derived forms are clean and count the same (asserted in
    the child); here: stages were examined against the nodes that stayed."""
    got = emulated["relax_whatifs"]
    assert "error" not in got, got
    assert sum(p["checked"][2] for p in got["plain"]) > 0 and sum(p["pairs_existing"] for p in got["plain"]) > 0, got["plain"]


@pytest.mark.parametrize("i", range(len(SC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    """tests/audit_stages_cases.py: each edit through the claimed form raises exactly the flags stated there, device and reference alike; the edits of (a) pass all six
    earlier passes clean, and so do the (b) edits of pods with two required terms, whose later stage is no relaxation of the earlier; the (b) edits of pods with a
    preference keep the first pass clean (the fourth flags them: there the last stage relaxes every earlier one)."""
    name, ok = emulated["tamper"][i]
    assert name == SC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


def test_every_bit_has_an_edit_the_six_earlier_passes_let_through():
    """Among the edits on which the matrix asserts the gate clean, (a) and (b) each hold one per bit."""
    res = {n: w for n, _, _, w in _matrix_wants()}
    for kind in ("(a)", "(b)"):
        bits = 0
        for n in SC.SILENT:
            if n.startswith(kind):
                for b in res[n].values():
                    bits |= b
        assert bits == SR.BITS["STAGE_EXISTING"] | SR.BITS["STAGE_TEMPLATE"], kind


def _matrix_wants():
    """the matrix's names and expected flags, from a result shaped as `check_genuine` demands (no solve needed to read them)"""
    res = {"n_existing": 2, "n_new": 1, "unscheduled": np.array([0], dtype=np.int32), "pod_node": np.array([-1, 0, 0, 0, 0, 2, 2, 0, 2], dtype=np.int32),
           "pod_stage": np.array([1, 0, 0, 0, 0, 0, 0, 0, 0], dtype=np.int32), "node_requests": np.zeros(1, dtype=np.int64)}
    prob = {"R": 1, "stage_cls": np.zeros(20, dtype=np.uint32), "pod_stage_off": np.arange(0, 20, 2, dtype=np.uint32), "cls_requests": np.zeros(1, dtype=np.int64)}
    return SC.tampers(res, np.array([-1, 0, 1, 2, 3, 4, 5, 6, 7], dtype=np.int32), prob)


@pytest.mark.parametrize("i", range(len(SC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == SC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
PLAIN, ZONE2, TEAM, NO_TEAM, PORTS, VOLUMES, NAMED, OWNER, HUGE = FC.CLASSES
E0, E1, E2, N0, N1, N2, N3 = FC.NODES
EX, TM, UN, SQ = SR.BITS["STAGE_EXISTING"], SR.BITS["STAGE_TEMPLATE"], SR.BITS["STAGE_UNRELAXED"], SR.BITS["SEQ"]


def _unit(name):
    """(problem, result, commit numbers, {pod: bits}, pods examined, stages examined, (class, node-or-template) pairs evaluated) over tests/audit_firstfit_cases.py's
    hand-made problem: six pods on e0 -- here pod 0 has a chain of two stages [first, PLAIN] and ended at stage 1, pods 1 .. 5 have the one stage PLAIN."""
    p, r, s = FC._tiny()
    EXISTING, TEMPLATES = 3, 2      # what one class is evaluated against: every existing node it is labelled for, the unlimited templates
    first, k, want, pods, stages, pairs = PLAIN, 1, {}, 1, 1, EXISTING + TEMPLATES
    if name == "an earlier stage an existing node and a template would have taken":
        want = {0: EX | TM}      # e0 has room for another plain pod; template 1 opens a machine for one
    elif name == "no pod relaxed: nothing is examined":
        k = 0; pods = stages = pairs = 0
    elif name == "a stage with a group is not examined":
        first, pods, stages, pairs = OWNER, 0, 0, 0
    elif name == "a stage with a port is not examined":
        first, pods, stages, pairs = PORTS, 0, 0, 0
    elif name == "a limited template never admits":
        first = HUGE      # no existing node holds 2 000 units; template 0 would, and is limited; templates 1 and 2 do
        want = {0: TM}
    elif name == "the same with the unlimited templates tainted: the limited one is all there is":
        first = HUGE; p["tmpl_taints"] = np.array([0, 1, 1], dtype=np.uint64)
    elif name == "an unlabelled key on the existing node: the pair is not examined":
        first, pairs = ZONE2, 2 + TEMPLATES      # e0 and e1 are in other zones; e2, Compatible with any zone, is not asked; a fresh machine in zone 2 admits
        want = {0: TM}
    elif name == "a class with volumes is not examined against existing nodes":
        first, pairs = VOLUMES, TEMPLATES
        want = {0: TM}
    elif name == "an existing node the result fills to the brim does not admit":
        p["en_avail"][:] = 600; p["tmpl_taints"] = np.array([0, 1, 1], dtype=np.uint64); r["pod_node"][:] = [E0, E0, E0, E0, E0, E0]      # six pods of 100 on e0: full; e1 and e2 have room
        want = {0: EX}
    elif name == "the same with every node full":
        p["en_avail"][:] = 200; p["tmpl_taints"] = np.array([0, 1, 1], dtype=np.uint64); r["pod_node"][:] = [E0, E0, E1, E1, E2, E2]
    elif name == "a removed what-if node is not asked":
        p["removed"] = [E0, E1, E2]; r["pod_node"][:] = N0; p["tmpl_taints"] = np.array([0, 1, 1], dtype=np.uint64); pairs = TEMPLATES
    elif name == "an unscheduled pod short of its chain's end":
        r["pod_node"][0] = -1; s[:] = [-1, 0, 1, 2, 3, 4]; r["unscheduled"] = np.array([0], dtype=np.int32)
        k = 0; want = {0: UN}; pods = stages = pairs = 0
    elif name == "an unscheduled pod at its chain's end is examined like a placed one":
        r["pod_node"][0] = -1; s[:] = [-1, 0, 1, 2, 3, 4]; r["unscheduled"] = np.array([0], dtype=np.int32); want = {0: EX | TM}
    elif name == "two pods with one commit number fail SEQ and are not examined":
        s[1] = s[0]; want = {0: SQ, 1: SQ}; pods = stages = pairs = 0
    elif name == "a stage outside the chain addresses nothing":
        k = 9; pods = stages = pairs = 0
    else:
        raise KeyError(name)
    p["pod_stage_off"] = np.array([0, 2, 3, 4, 5, 6, 7], dtype=np.uint32)
    p["stage_cls"] = np.array([first] + [PLAIN] * 6, dtype=np.uint32)
    r["pod_stage"][0] = k
    r["node_requests"] = np.zeros(4, dtype=np.int64)
    return p, r, s, want, pods, stages, pairs


UNIT = ["an earlier stage an existing node and a template would have taken", "no pod relaxed: nothing is examined", "a stage with a group is not examined", "a stage with a port is not examined",
        "a limited template never admits", "the same with the unlimited templates tainted: the limited one is all there is", "an unlabelled key on the existing node: the pair is not examined",
        "a class with volumes is not examined against existing nodes", "an existing node the result fills to the brim does not admit", "the same with every node full",
        "a removed what-if node is not asked", "an unscheduled pod short of its chain's end", "an unscheduled pod at its chain's end is examined like a placed one",
        "two pods with one commit number fail SEQ and are not examined", "a stage outside the chain addresses nothing"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, want, pods, stages, pairs = _unit(name)
    got = SR.audit(p, r, s)
    assert H.flagged(got["pod_flags"]) == want
    assert got["checked"] == [int((r["pod_node"] >= 0).sum()), pods, stages, pairs] and got["skipped_pods"] == 6 - pods, (got["checked"], got["skipped_pods"])
    assert (got["admitting_pairs"] > 0) == any(b & (EX | TM) for b in want.values())


def test_both_directions_have_unit_cases():
    wants = [_unit(n)[3] for n in UNIT]
    flagged = [w for w in wants if any(b & SR.STAGE for b in w.values())]
    assert len(flagged) >= 6 and len(UNIT) - len(flagged) >= 7
    assert {b for w in wants for b in w.values()} >= {EX, TM, EX | TM, UN, SQ}
