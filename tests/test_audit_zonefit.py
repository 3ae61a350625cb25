"""(CPU) The audit's ninth pass -- first-fit order for the pods under zonal spread (include/ksolve.h ks_audit_zonefit_dev, KS_AUDIT_POD_ZFIT_*) -- validated where a
correct result is known, before any GPU run:
  a) the soundness gate: the reference pass (tests/audit_zonefit_ref.py) over every result the fourth pass's gate audits (the emulator's committed cases through both
     pack kernels, the pack cases, the flattened what-ifs, the wide and the topology snapshot's what-ifs) and over the `zonal_cluster` seeds raises NO flag; a rule that
     flagged one of them would be a wrong rule, not a finding.  The kernels' own source (karpenter_core_amd/csrc/ks_audit_zonefit.inc) is compiled into the emulator
     build and runs beside the reference: the two agree bit for bit, every counter included; derived batches count what their flattened twins count;
  b) the tamper matrix, the claimed results with indices out of range and the kernels' other paths (tests/audit_zonefit_cases.py) on the emulator;
  c) unit cases of the reference alone on a hand-made problem: one per clause of the rule and direction.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import numpy as np
import pytest

import audit_firstfit_cases as FC
import audit_harness as H
import audit_zonefit_cases as ZC
import audit_zonefit_ref as ZR
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
import audit_zonefit_ref as ZR, audit_zonefit_cases as ZC, audit_harness as H
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR, test_whatif_derived as WD
out = {}
def audited(name, f, kinds=False):
    # the reference pass's findings (must be none), what it evaluated, and whether the emulated device pass says the same
    try:
        dev, flags = ZC.compare(S, f)
        out[name] = dict(ZC.summary(dev), device_agrees=True)
        if kinds:
            prob = ZR.problem_arrays(S, f)
            out[name]["pairs_by_kind"] = ZR.audit(prob, f.result_arrays(), H.commit_numbers(S, f, prob))["pairs_by_kind"]
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
for seed in json.loads(sys.argv[3]):
    for tag, fl in (("zonal", 0), ("zonal_no_rr", S.KS_FLAG_NO_RR)):
        f = S.FlatProblem(ZC.zonal_cluster(seed), flags=fl); f.solve(decode=False); audited("%%s/%%d" %% (tag, seed), f, kinds=True); f.close()
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
    for i, d in enumerate(S.audit_zonefit_batch(derived)):
        out[tag + "_derived/%%d" %% i] = dict(ZC.summary(d), device_agrees=True)
snap, pod_node, bound, _ = WR.wide_snapshot(**E.WIDE_SNAPSHOT)
both_forms("wide_whatifs", S.ParsedProblem(snap), pod_node, E.WIDE_SETS)
its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
both_forms("topology_whatifs", S.ParsedProblem(snap), pod_node, json.loads(sys.argv[2]))
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in ZC.run_tamper_matrix(S)]
out["range"] = [[n, ok if ok is True else str(ok)] for n, ok in ZC.run_range_cases(S)]
out["shapes"] = [[n, ok if ok is True else str(ok)[:600]] for n, ok in ZC.run_shapes(S)]
out["clauses"] = [[n, ok if ok is True else str(ok)[:600]] for n, ok in ZC.run_clauses(S)]
print("RESULT " + json.dumps(out))
"""

TOPOLOGY_SETS = H.WHATIF_SETS
WHATIFS, FLAT, DERIVED = H.gate_names()
ZONAL = ["%s/%d" % (tag, seed) for seed in ZC.SEEDS for tag in ("zonal", "zonal_no_rr")]
NAMES = FLAT + DERIVED + ZONAL


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [E.CASES, E.PACK_CASES], TOPOLOGY_SETS, ZC.SEEDS)


@pytest.mark.parametrize("name", NAMES)
def test_the_pass_flags_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["pods"] == {}, got["pods"]
    assert got["device_agrees"], got


def test_the_gate_is_not_vacuous(emulated):
    """Over the committed cases the rule examined pods, ran zone tests, evaluated the static predicate and found pairs that admit, with masks that are the reference's
    own numbers; the totals are DESIGN.md 7.32's."""
    tot = lambda names: (sum(emulated[n]["checked"][1] for n in names), sum(emulated[n]["checked"][2] for n in names), sum(emulated[n]["checked"][3] for n in names),
                         sum(emulated[n]["admitting"] for n in names), sum(emulated[n]["exact"] for n in names))
    print("committed cases: pods examined, pairs, passed the zone test, admitting, exact:", tot(FLAT))
    print("zonal_cluster seeds:", tot(ZONAL))
    assert all(x > 0 for x in tot(FLAT)), tot(FLAT)
    assert all(x > 0 for x in tot(ZONAL)), tot(ZONAL)


@pytest.mark.parametrize("name", ZONAL)
def test_every_seed_of_the_family_examines_pods_against_both_kinds_of_target(emulated, name):
    got = emulated[name]
    assert got["checked"][1] > 0 and got["admitting"] > 0 and got["exact"] > 0 and got["pairs_by_kind"][0] > 0 and got["pairs_by_kind"][1] > 0, got


@pytest.mark.parametrize("name", DERIVED)
def test_a_derived_whatif_counts_what_the_same_whatif_flattened_counts(emulated, name):
    d, p = emulated[name], emulated[name.replace("_derived", "")]
    same = lambda x: (x["checked"], x["admitting"], x["exact"], x["skipped"], x["mixed"], x["n_new"], x["n_placed"], x["groups"][0])
    assert same(d) == same(p), (d, p)


@pytest.mark.parametrize("i", range(len(ZC.TAMPER_NAMES)))
def test_tamper_matrix_on_the_emulator(emulated, i):
    name, ok = emulated["tamper"][i]
    assert name == ZC.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(ZC.RANGE_NAMES)))
def test_claimed_indices_out_of_range_on_the_emulator(emulated, i):
    """Flags or skips, as the reference -- which never reads past a table -- says; the same cases go to the GPU only in tests/test_audit_zonefit_gpu.py, after these."""
    name, ok = emulated["range"][i]
    assert name == ZC.RANGE_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(ZC.CLAUSE_NAMES)))
def test_the_clauses_of_the_new_node_predicate_on_the_emulator(emulated, i):
    """tests/audit_zonefit_cases.py run_clauses: the Fits pair and the taint pair of tests/audit_firstfit_cases.py through this pass's kernels."""
    name, ok = emulated["clauses"][i]
    assert name == ZC.CLAUSE_NAMES[i]
    assert ok is True, (name, ok)


@pytest.mark.parametrize("i", range(len(ZC.SHAPE_NAMES)))
def test_the_kernels_other_paths_on_the_emulator(emulated, i):
    name, ok = emulated["shapes"][i]
    assert name == ZC.SHAPE_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference pass alone, on a hand-made problem
PLAIN, PORTS, OWNER = FC.PLAIN, FC.PORTS, FC.OWNER
E0, E1, E2, N0, N3 = FC.E0, FC.E1, FC.E2, FC.N0, FC.N3
EX, NW = ZR.BITS["ZFIT_EXISTING"], ZR.BITS["ZFIT_NEW"]
ZONAL_G, HOSTNAME_G, FILTERED_G, INACTIVE_G, AFFINITY_G = range(5)      # the groups: 0 spread over the zone, maxSkew 1 | 1 hostname spread | 2 zonal spread under a node filter | 3 a zonal spread created later | 4 zonal affinity
SELF = 1 << 31


def _hand(name):
    """tests/audit_firstfit_cases.py's hand-made problem -- e0 in zone 0, e1 in zone 1, e2 without a label, 1 000 units to spare each; four new nodes; six pods of 100
    units on e0 in commit order -- with five topology groups; zones 0, 1 and 2 are registered with group 0 at a count of 0.  Pod 3 is the subject: of class OWNER, placed
    on e1 with commit number 3 although e0 has room for its requests -- flagged ZFIT_EXISTING unless a clause of the rule keeps e0 from admitting it at that moment.
    Returns (problem, result, commit numbers, {pod: bits}, pods examined, mixed pods)."""
    p, r, s = FC._tiny()
    C = p["C"]
    u32 = lambda x: np.array(x, dtype=np.uint32)
    count = np.full(5 * 64, -1, dtype=np.int32)
    for g in range(5):
        count[g * 64:g * 64 + 3] = 0
    p.update({"G": 5, "GH": 1, "grp_key": np.array([0, -2, 0, 0, 0], dtype=np.int32), "grp_type": np.array([0, 0, 0, 0, 1], dtype=np.uint8),
              "grp_active": np.array([1, 1, 1, 0, 1], dtype=np.uint8), "grp_max_skew": np.array([1, 1, 1, 1, 0], dtype=np.int32), "grp_count": count,
              "grp_hslot": np.array([-1, 0, -1, -1, -1], dtype=np.int32), "grph_count": np.zeros(p["E"], dtype=np.int32),
              "grp_filter_off": u32([0, 0, 0, 1, 1, 1]), "flt.present": u32([1]), "flt.it_state": np.array([0], dtype=np.int32)})
    own, sel, want, pods, mixed = {OWNER: [ZONAL_G]}, {}, {3: EX}, 1, 0
    cls, node = p["stage_cls"], r["pod_node"]
    cls[3], node[3] = OWNER, E1

    def zone_req(c, mask):
        p["cls.present"][c] |= 1
        p["cls.mask"][c * p["K"]] = mask
    if name == "every zone admits at s: e0 comes first":
        pass
    elif name == "U + self == maxSkew + 1 at s":
        own[OWNER] = [ZONAL_G | SELF]; sel[PLAIN] = [ZONAL_G]; want = {}      # pods 0, 1 and 2 were counted in zone 0 before it
    elif name == "the prefix decides, not the final counts":
        own[OWNER] = [ZONAL_G | SELF]; sel[PLAIN] = [ZONAL_G]; s[:] = [1, 2, 3, 0, 4, 5]      # claimed to have committed first: zone 0 was empty then
    elif name == "the minimum is taken among the pod's own domains: narrower, it is higher":
        own[OWNER] = [ZONAL_G | SELF]; count[0:3] = [1, 1, 0]; zone_req(OWNER, 0b011)      # among {0, 1}: 1 + 1 - 1 <= 1
    elif name == "the same counts with every zone among them":
        own[OWNER] = [ZONAL_G | SELF]; count[0:3] = [1, 1, 0]; want = {}      # 1 + 1 - 0 > 1
    elif name == "none of the pod's domains is registered":
        count[0:3] = [0, -1, 0]; zone_req(OWNER, 0b010); node[3] = E2; want = {}      # (on e2, which names no zone: e0 and e1 come first, and nothing is proved of them)
    elif name == "a wild recorder counts in every domain":
        sel[PLAIN] = [ZONAL_G]; node[0] = node[1] = E2; want = {}      # two pods on the node without a label: U + W = 2 > 1 in zone 0 (pod 2 is there too)
    elif name == "an existing node without the label is no target":
        p["en.present"][E0] = 0; want = {}
    elif name.startswith("an ineligible group beside the zonal one: "):
        what = name.split(": ")[1]
        own[OWNER] = [ZONAL_G, {"hostname spread": HOSTNAME_G, "a filtered zonal spread": FILTERED_G, "an inactive group": INACTIVE_G, "zonal affinity": AFFINITY_G}[what]]
        want, pods, mixed = {}, 0, 1 if what == "hostname spread" else 0
    elif name == "a class with host ports":
        cls[3] = PORTS; own = {PORTS: [ZONAL_G]}; want, pods = {}, 0
    elif name == "a class with five groups":
        own[OWNER] = [ZONAL_G] * 5; want, pods = {}, 0
    elif name == "a class with four groups":
        own[OWNER] = [ZONAL_G] * 4
    elif name == "a placed pod claimed unscheduled":
        node[3] = -1; s[:] = [0, 1, 2, -1, 3, 4]; r["unscheduled"] = np.array([3], dtype=np.int32)
    elif name in ("an opener passed over a machine opened before s", "the machine's zone was not one value before s", "the machine opened after s"):
        # pod 2 opens n0, which ends in zone 0; pod 3 opens n3, in zone 1.  Both are on new nodes: e0 would have taken either
        cls[2], node[2], node[3] = OWNER, N0, N3
        r["node_present"][0] |= 1; r["node_mask"][0][0] = 1; r["node_present"][3] |= 1; r["node_mask"][3][0] = 2
        want, pods = {2: EX, 3: EX | NW}, 2
        if name == "the machine's zone was not one value before s":
            cls[2] = PLAIN; want, pods = {3: EX}, 1      # a plain pod pins nothing: when n0 was narrowed to zone 0 is not known
        elif name == "the machine opened after s":
            s[:] = [0, 1, 3, 2, 4, 5]; want = {2: EX | NW, 3: EX}      # the roles change hands
    else:
        raise KeyError(name)
    off = lambda d: np.cumsum([0] + [len(d.get(c, [])) for c in range(C)]).astype(np.uint32)
    flat = lambda d: u32([x for c in range(C) for x in d.get(c, [])])
    p.update({"cls_own_off": off(own), "own_list": flat(own), "cls_sel_off": off(sel), "sel_list": flat(sel), "cls_isel_off": off({}), "isel_list": u32([]), "cls_iown_off": off({}), "iown_list": u32([])})
    r["node_requests"] = np.array([sum(int(p["cls_requests"][cls[q]]) for q in range(6) if node[q] == 3 + j) for j in range(4)], dtype=np.int64)
    return p, r, s, want, pods, mixed


UNIT = ["every zone admits at s: e0 comes first", "U + self == maxSkew + 1 at s", "the prefix decides, not the final counts",
        "the minimum is taken among the pod's own domains: narrower, it is higher", "the same counts with every zone among them", "none of the pod's domains is registered",
        "a wild recorder counts in every domain", "an existing node without the label is no target", "an ineligible group beside the zonal one: hostname spread",
        "an ineligible group beside the zonal one: a filtered zonal spread", "an ineligible group beside the zonal one: an inactive group", "an ineligible group beside the zonal one: zonal affinity",
        "a class with host ports", "a class with five groups", "a class with four groups", "a placed pod claimed unscheduled", "an opener passed over a machine opened before s",
        "the machine's zone was not one value before s", "the machine opened after s"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_pass_on_a_hand_made_result(name):
    p, r, s, want, pods, mixed = _hand(name)
    out = ZR.audit(p, r, s)
    flags = out["pod_flags"]
    assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == want
    placed = 5 if name == "a placed pod claimed unscheduled" else 6
    assert out["checked"][0] == placed and out["checked"][1] == pods and out["skipped_pods"] == 6 - pods and out["mixed_pods"] == mixed, out
    assert (out["eligible_groups"], out["skipped_groups"]) == (1, 4)
    assert (out["checked"][2] > 0) if pods else (out["checked"][2] == out["checked"][3] == out["admitting_pairs"] == 0), out


def test_the_silent_clauses_and_their_counterparts_are_both_there():
    flagged = [n for n in UNIT if _hand(n)[3]]
    assert len(flagged) == 8 and len(UNIT) - len(flagged) == 11
