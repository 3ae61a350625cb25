"""(CPU) The audit's invariants, validated where a correct result is known: the reference audit (tests/audit_ref.py) over every result the lane-fibre emulator returns
for its committed cases (tests/test_rr_emulated.py: the register-resident kernel's, ks_pack's, the what-if batches') -- results proven equal to the oracle's there --
must find NOTHING, on every case; a check that flags one of them would be a wrong definition of that check, not a finding.  The audit kernels' own source
(karpenter_core_amd/csrc/ks_audit.inc) is compiled into the emulator build too and runs beside the reference: the two agree bit for bit, on the genuine results and on
the tamper matrix (tests/audit_cases.py).  And unit cases of the reference audit alone on hand-made results, one per bit.  Runs the emulator in a subprocess: its build
replaces the two libraries for the whole process (tests/simlib.py)."""
import numpy as np
import pytest

import audit_harness as H
import audit_ref as A
import test_rr_emulated as E

CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
from karpenter_core_amd import workloads as W
import audit_ref as A, audit_cases as C
import test_fuzz_mid as T, test_fuzz_rr as R, test_rr_emulated as E, test_wide_resources as WR
out = {}
def bits(flags, names):
    return {k: int(((flags & v) != 0).sum()) for k, v in names.items() if ((flags & v) != 0).any()}
def audited(name, f):
    # the reference audit's findings (must be none), and whether the emulated device audit says the same
    try:
        dev = f.audit()
        pf, nf = A.audit(A.problem_arrays(S, f), f.result_arrays())
        out[name] = {"pods": bits(pf, A.POD), "nodes": bits(nf, A.NODE), "P": int(len(pf)), "n_new": dev["n_new"],
                     "device_agrees": bool(np.array_equal(pf, dev["pod_flags"]) and np.array_equal(nf, dev["node_flags"]))}
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
rr_cases, pack_cases = json.loads(sys.argv[1])
for name, kind, args in rr_cases:
    p = R.rr_problem(args["seed"]) if kind == "rr" else T.mid_problem_wide(args["seed"]) if kind == "wide" else (getattr(W, kind)(**args) if kind != "mid" else T.mid_problem(args["seed"]))
    f = S.FlatProblem(p); f.solve(decode=False); audited("rr/" + name, f); f.close()
for name, kind, args, no_rr in pack_cases:
    f = S.FlatProblem(E._problem(kind, args), flags=S.KS_FLAG_NO_RR if no_rr else 0); f.solve(decode=False); audited("pack/" + name, f); f.close()
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
# derived on the device: no flattening of their own to restate the audit over -- the device audit of the batch, which must find what the reference found above: nothing
derived = S.open_whatifs(parsed, pod_node, E.WIDE_SETS, derive=True)
S.solve_batch_resident(derived)
for i, d in enumerate(S.audit_batch(derived)):
    out["wide_whatifs_derived/%%d" %% i] = {"pods": bits(d["pod_flags"], A.POD), "nodes": bits(d["node_flags"], A.NODE), "P": int(len(d["pod_flags"])), "n_new": d["n_new"], "device_agrees": True}
out["tamper"] = [[n, ok if ok is True else str(ok)] for n, ok in C.run_tamper_matrix(S)]
print("RESULT " + json.dumps(out))
"""

NAMES = ["rr/" + c[0] for c in E.CASES] + ["pack/" + c[0] for c in E.PACK_CASES] + ["whatifs/%d" % i for i in range(4)] + \
        ["wide_whatifs/%d" % i for i in range(len(E.WIDE_SETS))] + ["wide_whatifs_derived/%d" % i for i in range(len(E.WIDE_SETS))]


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [E.CASES, E.PACK_CASES])


@pytest.mark.parametrize("name", NAMES)
def test_the_audit_finds_nothing_in_a_result_equal_to_the_oracles(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["pods"] == {} and got["nodes"] == {}, got
    assert got["device_agrees"], got


def test_the_cases_reach_new_nodes_and_existing_ones(emulated):
    assert sum(1 for n in NAMES if emulated[n].get("n_new", 0) > 0) > 40 and emulated["rr/config3_3500"]["P"] == 3500


@pytest.mark.parametrize("i", range(15))
def test_tamper_matrix_on_the_emulator(emulated, i):
    """tests/audit_cases.py: one minimal edit per bit through the claimed form -- exactly that bit on exactly those indices, from the kernels' source and from the reference."""
    import audit_cases as C
    name, ok = emulated["tamper"][i]
    assert name == C.TAMPER_NAMES[i]
    assert ok is True, (name, ok)


# ---------------------------------------------------------------------------------------------------------------- the reference audit alone, on hand-made results
def _tiny():
    """One key (the zone, two values, well known), one resource, two types, one template without limits, one existing node (zone 0, taint 0, hostname 0, a reservation of
    port 80, one volume driver with room for one claim), four classes: 0 plain (tolerates everything), 1 tolerates nothing, 2 zone In [1], 3 hostname In [nowhere] with
    port 80, the failed-volume entry and claim 0 of the driver."""
    p = {"P": 4, "C": 4, "T": 2, "M": 1, "E": 1, "K": 1, "R": 1, "S": 1, "SC": 1, "max_new_nodes": 4, "wellknown_mask": 1, "key_zone": 0, "key_ct": -1, "n_ct": 1, "ND": 1, "SW": 1}
    u32, u64, i32, i64 = (lambda *x: np.array(x, dtype=np.uint32)), (lambda *x: np.array(x, dtype=np.uint64)), (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.int64))
    p.update({"key_nvalues": u32(2), "value_int": np.full(64, -2 ** 31, dtype=np.int32), "it_present": u32(1, 1), "it_complement": u32(0, 0), "it_mask": u64(3, 1), "it_offer": u64(3, 1),
              "it_alloc": i64(10, 100), "its_fail": np.zeros(1, dtype=np.uint8), "its_types": u64(3), "tmpl_taints": u64(0), "tmpl_types": u64(3), "tmpl_daemon": i64(1),
              "tmpl_daemon_present": u32(1), "tmpl_limit_present": u32(0xFFFFFFFF), "en_taints": u64(1), "en_avail": i64(5), "en_requests": i64(1), "en_requests_present": u32(1),
              "en_port_off": u32(0, 1), "cls_hn_mode": np.array([0, 0, 0, 1], dtype=np.uint8), "cls_hn_off": u32(0, 0, 0, 0, 0), "hn_list": u32(), "cls_requests": i64(2, 2, 2, 2),
              "cls_requests_present": u32(1, 1, 1, 1), "cls_tolerated": u64(1, 0, 1, 1), "cls_port_off": u32(1, 1, 1, 1, 2), "ports": u64(80 << 32, 80 << 32),
              "en_vol_limit": i32(1), "en_vol_count": i32(1), "en_vol_set": u64(0), "cls_vol_off": u32(0, 0, 0, 0, 2), "vol_list": u32(0, 0xFFFFFFFF), "pod_stage_off": u32(0, 1, 2, 3, 4),
              "stage_cls": u32(0, 1, 2, 3)})
    for fam, n, present, mask in (("tmpl", 1, [0], [0]), ("en", 1, [1], [1]), ("cls", 4, [0, 0, 1, 0], [0, 0, 2, 0])):
        p.update({fam + ".present": np.array(present, dtype=np.uint32), fam + ".complement": np.zeros(n, dtype=np.uint32), fam + ".mask": np.array(mask, dtype=np.uint64),
                  fam + ".gt": np.full(n, A.NOGT, dtype=np.int32), fam + ".lt": np.full(n, A.NOLT, dtype=np.int32), fam + ".it_state": np.zeros(n, dtype=np.int32)})
    # pod 0 on the existing node, pod 1 alone on new node 0 (3 = its 2 + the daemon's 1; both types fit and offer), pods 2 and 3 unscheduled
    r = {"n_existing": 1, "n_new": 1, "pod_node": i32(0, 1, -1, -1), "pod_stage": i32(0, 0, 0, 0), "pod_seq": i32(0, 1, -1, -1), "unscheduled": i32(2, 3), "node_tmpl": i32(0),
         "node_types": u64(3).reshape(1, 1), "node_requests": i64(3).reshape(1, 1), "node_requests_present": u32(1), "node_present": u32(0), "node_complement": u32(0),
         "node_mask": u64(0).reshape(1, 1), "node_gt": np.full((1, 1), A.NOGT, dtype=np.int32), "node_lt": np.full((1, 1), A.NOLT, dtype=np.int32), "node_it_state": i32(0)}
    return p, r


def _place(r, pod, node, seq):
    r["pod_node"][pod], r["pod_seq"][pod] = node, seq
    r["unscheduled"] = np.array([u for u in r["unscheduled"] if u != pod], dtype=np.int32)


def _edit(name):
    p, r = _tiny()
    pods, nodes = {}, {}
    if name == "clean":
        pass
    elif name == "RANGE":
        r["pod_node"][0] = 2; pods = {0: A.POD["RANGE"]}
    elif name == "RANGE seq":
        r["pod_seq"][2] = 5; pods = {2: A.POD["RANGE"]}
    elif name == "UNSCHEDULED_LIST":
        r["unscheduled"] = np.array([2, 3, 3], dtype=np.int32); pods = {3: A.POD["UNSCHEDULED_LIST"]}
    elif name == "TAINTS":
        r["pod_node"][1] = 0; pods = {1: A.POD["TAINTS"]}; nodes = {1: A.NODE["EMPTY"]}
    elif name == "REQUIREMENTS":
        _place(r, 2, 0, 2); pods = {2: A.POD["REQUIREMENTS"]}                                  # zone In [1] on the node of zone 0
    elif name == "HOSTNAME PORTS VOLUME_ERROR VOLUMES":
        _place(r, 3, 0, 2); pods = {3: A.POD["HOSTNAME"] | A.POD["PORTS"] | A.POD["VOLUME_ERROR"]}; nodes = {0: A.NODE["VOLUMES"]}      # its port 80 meets the node's reservation, its claim the full driver
    elif name == "PORTS between pods":
        p["stage_cls"][1] = 3; p["cls_hn_mode"][3] = 0; p["cls_vol_off"][4] = 0; p["stage_cls"][0] = 3; r["pod_node"][0] = 1
        pods = {0: A.POD["PORTS"], 1: A.POD["PORTS"]}; r["node_requests"][0, 0] = 5
    elif name == "RESOURCES":
        p["en_avail"][0] = 2; nodes = {0: A.NODE["RESOURCES"]}                                  # 1 + 2 > 2
    elif name == "EMPTY":
        _place(r, 1, -1, -1); r["pod_node"][1], r["pod_seq"][1] = -1, -1; r["unscheduled"] = np.array([2, 3, 1], dtype=np.int32); nodes = {1: A.NODE["EMPTY"]}
    elif name == "TEMPLATE":
        r["node_tmpl"][0] = 1; nodes = {1: A.NODE["TEMPLATE"]}
    elif name == "REQUESTS":
        r["node_requests"][0, 0] = 4; nodes = {1: A.NODE["REQUESTS"]}
    elif name == "OPTIONS_EMPTY":
        r["node_types"][0, 0] = 0; nodes = {1: A.NODE["OPTIONS_EMPTY"] | A.NODE["OPTIONS_MISSING"]}
    elif name == "OPTIONS_EXTRA outside T":
        r["node_types"][0, 0] = 7; nodes = {1: A.NODE["OPTIONS_EXTRA"]}
    elif name == "OPTIONS_EXTRA too small":
        p["it_alloc"][0] = 2; nodes = {1: A.NODE["OPTIONS_EXTRA"]}                              # 3 > 2
    elif name == "OPTIONS_EXTRA no offering":
        r["node_present"][0] = 1; r["node_mask"][0, 0] = 2; nodes = {1: A.NODE["OPTIONS_EXTRA"]}      # the node narrowed to zone 1: type 1 has neither the value nor an offering there
    elif name == "OPTIONS_MISSING":
        r["node_types"][0, 0] = 1; nodes = {1: A.NODE["OPTIONS_MISSING"]}
    elif name == "OPTIONS_MISSING limited":
        r["node_types"][0, 0] = 1; p["tmpl_limit_present"][0] = 1
    return p, r, pods, nodes


UNIT = ["clean", "RANGE", "RANGE seq", "UNSCHEDULED_LIST", "TAINTS", "REQUIREMENTS", "HOSTNAME PORTS VOLUME_ERROR VOLUMES", "PORTS between pods", "RESOURCES", "EMPTY", "TEMPLATE",
        "REQUESTS", "OPTIONS_EMPTY", "OPTIONS_EXTRA outside T", "OPTIONS_EXTRA too small", "OPTIONS_EXTRA no offering", "OPTIONS_MISSING", "OPTIONS_MISSING limited"]


@pytest.mark.parametrize("name", UNIT)
def test_reference_audit_on_a_hand_made_result(name):
    p, r, pods, nodes = _edit(name)
    pf, nf = A.audit(p, r)
    assert {int(i): int(pf[i]) for i in np.nonzero(pf)[0]} == pods
    assert {int(i): int(nf[i]) for i in np.nonzero(nf)[0]} == nodes


def test_every_bit_has_a_unit_case():
    seen_p = seen_n = 0
    for name in UNIT:
        _, _, pods, nodes = _edit(name)
        for b in pods.values():
            seen_p |= b
        for b in nodes.values():
            seen_n |= b
    assert seen_p == sum(A.POD.values()) and seen_n == sum(A.NODE.values())
