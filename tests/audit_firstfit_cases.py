"""What tests/test_audit_firstfit.py (on the lane-fibre emulator) and tests/test_audit_firstfit_gpu.py (on the device) share: the comparison of the audit's fourth
pass with its reference (tests/audit_firstfit_ref.py, through tests/audit_harness.py), the hand-made problems -- generic pods over existing nodes, new nodes and two templates, where the reference's
first fit is known from how the problem was made --, the tamper matrix and the shapes at which the kernels take another path.  Every function takes the scheduler
module `S` it is to go through (the HIP libraries' or the emulator's)."""
import copy

import numpy as np

import audit_cases as C
import audit_ref as A
import audit_firstfit_ref as FR
import audit_harness as H
from audit_harness import _claimable, flagged
import audit_topo_cases as TC
from karpenter_core_amd import fake
from karpenter_core_amd.model import LABEL_INSTANCE_TYPE, Problem

B = FR.BITS
D = H.PASSES["firstfit"]      # the pass, and its comparison with the reference (tests/audit_harness.py)
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary
FIT = B["FIT_EXISTING"] | B["FIT_NEW"] | B["FIT_TEMPLATE"]


def with_generic_pods(pr: Problem, n: int = 3) -> Problem:
    """`pr` with a few pods under no constraint at all at the end of its list: whatever else the problem holds, some pod of it is examined."""
    pr = copy.copy(pr)
    pr.pods = list(pr.pods) + [TC._pod("zz-generic-%d" % i, cpu="10m", mem="8Mi") for i in range(n)]
    return pr


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix
TAMPER_NAMES = ["a generic pod moved to a later existing node with room", "the last pod of a new node claimed as the opener of an added node",
                "a placed generic pod claimed unscheduled", "an opener's node re-templated to the heavier template", "two pods given one commit number"]
N_PLAIN, N_BIG = 6, 3
BIG_TYPE = "fake-it-5"


def _small(name, zone):
    return C._node(name, zone, "2")      # 2 cores available: the plain pods fit, a big pod does not


def tamper_problem() -> Problem:
    """Two existing nodes with two cores to spare each, two provisioners without limits (`open` before `second`), and pods under no topology constraint: six of 100m --
    first fit puts them all on e0 -- and three of 2.5 cores that name the six-core type: no existing node holds one, the first opens a machine of `open`, the second
    joins it, the third opens another."""
    its = fake.instance_types(6)
    provs = [fake.provisioner("open", len(its), weight=10), fake.provisioner("second", len(its), weight=1)]
    pods = [TC._pod("big-%d" % i, cpu="2500m", mem="1Gi", node_selector={LABEL_INSTANCE_TYPE: BIG_TYPE}) for i in range(N_BIG)] + [TC._pod("plain-%d" % i) for i in range(N_PLAIN)]
    return Problem(instance_types=its, provisioners=provs, pods=pods, nodes=[_small("e0", C.Z1), _small("e1", C.Z2)], extra_well_known=fake.EXTRA_WELL_KNOWN)


def check_genuine(res, seq):
    """The genuine result is the one `tamper_problem` describes; returns (the big pods in commit order, the plain pods)."""
    big, plain = list(range(N_BIG)), list(range(N_BIG, N_BIG + N_PLAIN))
    assert res["n_existing"] == 2 and res["n_new"] == 2 and not len(res["unscheduled"]), (res["n_existing"], res["n_new"], res["unscheduled"])
    assert all(int(res["pod_node"][p]) == 0 for p in plain), res["pod_node"]
    big.sort(key=lambda p: int(seq[p]))
    assert [int(res["pod_node"][p]) for p in big] == [2, 2, 3] and list(res["node_tmpl"]) == [0, 0], (res["pod_node"], res["node_tmpl"])
    assert sorted(int(s) for s in seq) == list(range(N_BIG + N_PLAIN))
    return big, plain


def tampers(res, seq, prob):
    """[(name, edited copy of `res`, edited copy of `seq`, the tampered pod, the bits it must carry, True if nothing else may be flagged)]"""
    big, plain = check_genuine(res, seq)
    R, K, TW = prob["R"], prob["K"], (prob["T"] + 63) // 64
    out = []

    def case(name):
        r, s = _claimable(res), np.array(seq, dtype=np.int32)
        out.append([name, r, s, None, 0, False])
        return r, s, out[-1]
    r, s, o = case(TAMPER_NAMES[0])      # e0 still has room for it
    r["pod_node"][plain[2]] = 1
    o[3:] = [plain[2], B["FIT_EXISTING"], True]
    r, s, o = case(TAMPER_NAMES[1])      # the second big pod leaves node 2 for an added node 4 of the same template and type: node 2, opened earlier, has room again
    q = big[1]
    c = int(prob["stage_cls"][int(prob["pod_stage_off"][q]) + int(r["pod_stage"][q])])
    req = np.asarray(r["node_requests"], dtype=np.int64).reshape(-1, R).copy()
    mine = prob["cls_requests"][c * R:(c + 1) * R].astype(np.int64)
    tmpl = int(r["node_tmpl"][0])
    added = prob["tmpl_daemon"][tmpl * R:(tmpl + 1) * R].astype(np.int64) + mine
    req[0] -= mine
    r["node_requests"] = np.concatenate([req, added[None, :]]).reshape(-1)
    for name, width in (("node_tmpl", 1), ("node_types", TW), ("node_requests_present", 1), ("node_present", 1), ("node_complement", 1), ("node_mask", K), ("node_gt", K), ("node_lt", K),
                        ("node_it_state", 1)):
        a = np.asarray(r[name]).reshape(-1, width)
        r[name] = np.concatenate([a, a[0:1]]).reshape(-1)      # (every big pod is of one class: the added node's requirements, presence masks and options are node 2's)
    r["n_new"] = 3
    r["pod_node"][q] = 4
    o[3:] = [q, B["FIT_NEW"], False]      # (the third big pod opened its machine while node 2 -- as claimed -- had room: the reference says so too)
    r, s, o = case(TAMPER_NAMES[2])      # e0 and e1, node 3 (one big pod on six cores) and a fresh machine would all take it
    q = plain[4]
    r["pod_node"][q] = -1
    s[s > s[q]] -= 1
    s[q] = -1
    r["unscheduled"] = np.array([q], dtype=np.int32)
    o[3:] = [q, FIT, True]
    r, s, o = case(TAMPER_NAMES[3])      # template 0 takes the first big pod on a fresh machine: it cannot have opened one of template 1
    r["node_tmpl"][0] = 1
    o[3:] = [big[0], B["FIT_TEMPLATE"], False]
    r, s, o = case(TAMPER_NAMES[4])
    s[plain[1]] = s[plain[0]]
    o[3:] = [plain[0], B["SEQ"], False]
    assert [x[0] for x in out] == TAMPER_NAMES
    return out


def _verdict(S, flat, claimed, s, pod, bits, alone):
    try:
        dev, flags = compare(S, flat, claimed, s)
    except AssertionError as e:
        return "device and reference differ: %s" % (e,)
    got = flagged(dev["pod_flags"])
    if got.get(pod) != bits:
        return "pod %d carries %s, expected %d: %s" % (pod, got.get(pod), bits, got)
    if alone and set(got) != {pod}:
        return "flags %s, expected pod %d alone" % (got, pod)
    return True


def run_tamper_matrix(S):
    """Solve `tamper_problem`, audit the genuine result (clean) and every edit through the claimed form; returns [(name, True or what differs)]."""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    assert flat.dims["M"] == 2 and dev["skipped_pods"] == 0 and dev["checked"]["PODS"] == N_BIG + N_PLAIN and dev["admitting_pairs"] > 0, dev
    res, seq, prob = flat.result_arrays(), flat.pod_seq(), FR.problem_arrays(S, flat)
    report = []
    for name, claimed, s, pod, bits, alone in tampers(res, seq, prob):
        ok = _verdict(S, flat, claimed, s, pod, bits, alone)
        if ok is True and name == TAMPER_NAMES[1]:      # the edit is consistent: the first pass finds nothing in it
            first = flat.audit(claimed)
            if first["n_pods_flagged"] or first["n_nodes_flagged"]:
                ok = "the first pass flags the edit: %s %s" % (first["pod_bit_count"], first["node_bit_count"])
        if ok is True and name == TAMPER_NAMES[4]:      # SEQ and nothing else, on both pods
            got = flagged(flat.audit_firstfit(claimed, s)["pod_flags"])
            if sorted(got.values()) != [B["SEQ"], B["SEQ"]]:
                ok = "flags %s, expected SEQ on two pods" % (got,)
        report.append((name, ok))
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- shapes where the kernels take another path
TYPE_SHAPES = [(1, 0), (64, 63), (65, 64), (130, 129)]
NODE_SHAPES = [(65, 0), (65, 63), (257, 0), (257, 255)]
SHAPE_NAMES = ["T = %d: the only admitting type at bit %d" % ts for ts in TYPE_SHAPES] + ["E = 0", "n_new = 0", "P = 1 and exactly one used class", "257 used classes"] + \
              ["E = %d: the only admitting node at index %d" % ns for ns in NODE_SHAPES] + ["a node with 1 100 pods", "12 resource names", "two templates"]


def one_type_fits(T: int) -> Problem:
    """The ladder of T types -- type i has i + 1 cores -- and one pod that only the largest holds."""
    its = fake.instance_types(T)
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=[TC._pod("wide", cpu="%dm" % (T * 1000 - 500), mem="64Mi")], nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def one_node_fits(E: int, at: int) -> Problem:
    """E existing nodes, all full but node `at`, and two pods."""
    its = fake.instance_types(4)
    nodes = [TC._roomy("e%03d" % i, C.Z1) if i == at else C._node("e%03d" % i, C.Z1, "50m") for i in range(E)]
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=[TC._pod("p0"), TC._pod("p1")], nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def many_classes(n: int) -> Problem:
    """n pods of n different requests on two roomy existing nodes: n classes, all on e0."""
    its = fake.instance_types(4)
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=[TC._pod("c%03d" % i, cpu="%dm" % (i + 1)) for i in range(n)],
                   nodes=[TC._roomy("e0", C.Z1), TC._roomy("e1", C.Z2)], extra_well_known=fake.EXTRA_WELL_KNOWN)


def crowded_node(n: int) -> Problem:
    """n + 1 pods of one millicore; e0 has exactly n millicores to spare, e1 is roomy: n on e0, the last on e1 -- which is right only if e0's sum is n to the unit."""
    its = fake.instance_types(4)
    e0 = TC._roomy("e0", C.Z1)
    e0.available = {"cpu": "%dm" % n, "memory": "64Gi", "pods": "2000"}
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=[TC._pod("m%04d" % i, cpu="1m", mem="1Mi") for i in range(n + 1)],
                   nodes=[e0, TC._roomy("e1", C.Z2)], extra_well_known=fake.EXTRA_WELL_KNOWN)


def wide_problem() -> Problem:
    from karpenter_core_amd import workloads as W
    return with_generic_pods(W.wide_catalogue(names=12, pods=60, types=10, existing=4, seed=3, dense=True))


def run_shapes(S):
    """[(name, True or what differs)] -- each shape solved (clean by device and reference) and, where it says so, one claimed edit."""
    report = []

    def shape(name, make, body):
        flat = S.FlatProblem(make())
        try:
            flat.solve(decode=False)
            dev = assert_clean(S, flat)
            ok = body(flat, dev)
        except AssertionError as e:
            ok = "%s" % (e,)
        flat.close()
        report.append((name, ok))

    def claim(flat, edit):
        res, seq = _claimable(flat.result_arrays()), np.array(flat.pod_seq(), dtype=np.int32)
        edit(res, seq)
        dev, flags = compare(S, flat, res, seq)
        return flagged(flags)

    def last_type(T, bit):
        def body(flat, dev):
            res = flat.result_arrays()
            words = np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, (T + 63) // 64)
            assert flat.dims["T"] == T and res["n_new"] == 1 and [int(w) for w in words[0]] == [(1 << (bit % 64)) if i == bit // 64 else 0 for i in range(words.shape[1])], (flat.dims, words)
            assert dev["checked"] == {"SEQ": 1, "PODS": 1, "PAIRS": 2} and dev["admitting_pairs"] == 1, dev      # the fresh machine admits; the pod's own, with the pod on it, does not

            def unschedule(r, s):
                r["pod_node"][0], s[0], r["unscheduled"] = -1, -1, np.array([0], dtype=np.int32)
            got = claim(flat, unschedule)      # the walk over the types must reach the one bit to say so
            assert got == {0: B["FIT_TEMPLATE"]}, got
            return True
        return body
    for (T, bit), name in zip(TYPE_SHAPES, SHAPE_NAMES):
        shape(name, lambda T=T: one_type_fits(T), last_type(T, bit))
    shape("E = 0", lambda: TC.plain(3), lambda flat, dev: True if flat.dims["E"] == 0 and dev["n_new"] == 1 and dev["checked"] == {"SEQ": 3, "PODS": 3, "PAIRS": 2} else str(dev))
    shape("n_new = 0", lambda: TC.plain(3, True), lambda flat, dev: True if dev["n_new"] == 0 and dev["checked"] == {"SEQ": 3, "PODS": 3, "PAIRS": 2} and dev["admitting_pairs"] == 2 else str(dev))
    shape("P = 1 and exactly one used class", lambda: TC.plain(1), lambda flat, dev: True if flat.dims["P"] == 1 and dev["checked"] == {"SEQ": 1, "PODS": 1, "PAIRS": 2} else str(dev))

    def classes_257(flat, dev):
        assert flat.dims["C"] >= 257 and dev["checked"] == {"SEQ": 257, "PODS": 257, "PAIRS": 257 * 3} and dev["admitting_pairs"] == 257 * 3 and dev["n_new"] == 0, dev

        def move(r, s):
            r["pod_node"][256] = 1
        got = claim(flat, move)      # the class past the scan tile finds its own row of the first_* tables
        assert got == {256: B["FIT_EXISTING"]}, got
        return True
    shape("257 used classes", lambda: many_classes(257), classes_257)

    def only_node(E, at):
        def body(flat, dev):
            res = flat.result_arrays()
            assert flat.dims["E"] == E and [int(x) for x in res["pod_node"]] == [at, at] and dev["checked"]["PAIRS"] == E + 1 and dev["admitting_pairs"] == 2, (res["pod_node"], dev)

            def move(r, s):
                r["pod_node"][1] = E - 1
            got = claim(flat, move)      # the minimum over the existing nodes crosses lanes, waves and workgroups
            assert got == {1: B["FIT_EXISTING"]}, got
            return True
        return body
    for (E, at), name in zip(NODE_SHAPES, SHAPE_NAMES[8:12]):
        shape(name, lambda E=E, at=at: one_node_fits(E, at), only_node(E, at))

    def crowd(flat, dev):
        where = np.asarray(flat.result_arrays()["pod_node"])
        assert int((where == 0).sum()) == 1100 and int((where == 1).sum()) == 1 and dev["checked"] == {"SEQ": 1101, "PODS": 1101, "PAIRS": 3} and dev["admitting_pairs"] == 2, (dev, (where == 0).sum())
        return True
    shape("a node with 1 100 pods", lambda: crowded_node(1100), crowd)
    shape("12 resource names", wide_problem, lambda flat, dev: True if flat.dims["R"] == 12 and dev["checked"]["PODS"] >= 3 and dev["admitting_pairs"] > 0 else str((flat.dims, dev)))
    shape("two templates", tamper_problem, lambda flat, dev: True if flat.dims["M"] == 2 and dev["checked"]["PAIRS"] == 2 * (2 + 2 + 2) else str(dev))
    assert [r[0] for r in report] == SHAPE_NAMES
    return report


# ---------------------------------------------------------------------------------------------------------------- the hand-made problem of the reference's unit cases
CLASSES = PLAIN, ZONE2, TEAM, NO_TEAM, PORTS, VOLUMES, NAMED, OWNER, HUGE = range(9)
NODES = E0, E1, E2, N0, N1, N2, N3 = range(7)


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


# ---------------------------------------------------------------------------------------------------------------- the clauses of admits_new / admits_template, through the kernels
# Pairs of claimed results of one small solved problem each: the two of a pair differ in the one clause under test; in the first the reference raises no FIT_NEW /
# FIT_TEMPLATE bit on the target pod, in the second exactly that bit.  tests/audit_hostfit_cases.py and tests/audit_zonefit_cases.py run pairs of their own through
# `run_clause_pairs` with their pass's compare.
from karpenter_core_amd.model import Expr, Taint, Toleration      # noqa: E402

SIX_CORES = {LABEL_INSTANCE_TYPE: BIG_TYPE}      # the one type the clause problems' nodes end with: a walk over the types that admits, admits through it


def clause_problem(pods, provs=None, nodes=()) -> Problem:
    its = fake.instance_types(6)
    return Problem(instance_types=its, provisioners=provs or [fake.provisioner("open", len(its))], pods=list(pods), nodes=list(nodes), extra_well_known=fake.EXTRA_WELL_KNOWN)


def six_core_pod(uid, cpu, selector=None, **kw):
    return TC._pod(uid, cpu=cpu, mem="1Gi", node_selector=dict(selector or {}, **SIX_CORES), **kw)


def class_of(prob, r, p):
    return int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + int(r["pod_stage"][p])])


def new_node_of(prob, r, p):
    j = int(r["pod_node"][p]) - prob["E"]
    assert 0 <= j < int(r["n_new"]), (p, r["pod_node"])
    return j


def custom_key(prob, c):
    """the one key class c names that is no well-known label"""
    bits = int(prob["cls.present"][c]) & ~int(prob["wellknown_mask"])
    assert bits and not bits & (bits - 1), bits
    return bits.bit_length() - 1


def copy_key(r, prob, k, src, dst):
    """new node dst's final requirement on key k becomes new node src's"""
    K = prob["K"]
    for name in ("node_present", "node_complement"):
        a = np.asarray(r[name]).copy()
        a[dst] = (int(a[dst]) & ~(1 << k)) | (int(a[src]) & (1 << k))
        r[name] = a
    for name in ("node_mask", "node_gt", "node_lt"):
        a = np.asarray(r[name]).reshape(-1, K).copy()
        a[dst, k] = a[src, k]
        r[name] = a.reshape(-1)


def opened_in_order(r, s, prob, first, target):
    """`first` and `target` opened a new node each, `first` its own the earlier: the nodes"""
    j0, j1 = new_node_of(prob, r, first), new_node_of(prob, r, target)
    on = lambda j: [int(s[p]) for p in range(prob["P"]) if int(r["pod_node"][p]) == prob["E"] + j]
    assert j0 != j1 and min(on(j0)) == int(s[first]) < int(s[target]) == min(on(j1)), (r["pod_node"], s)
    return j0, j1


def boundary_requests(r, prob, j, c, past):
    """new node j ends with ONE type; its requests on the one resource that kept a pod of class c out are set so that need == that type's allocatable (+ `past`)"""
    R, T = prob["R"], prob["T"]
    words = np.asarray(r["node_types"], dtype=np.uint64).reshape(int(r["n_new"]), -1)[j]
    bits = [w * 64 + b for w in range(len(words)) for b in range(64) if (int(words[w]) >> b) & 1]
    assert len(bits) == 1, bits
    req = np.asarray(r["node_requests"], dtype=np.int64).reshape(-1, R).copy()
    mine = prob["cls_requests"][c * R:(c + 1) * R].astype(np.int64)
    alloc = np.array([int(prob["it_alloc"][x * T + bits[0]]) for x in range(R)], dtype=np.int64)
    over = [x for x in range(R) if req[j][x] + mine[x] > alloc[x]]
    assert len(over) == 1 and (int(r["node_requests_present"][j]) >> over[0]) & 1, (over, req[j], mine, alloc)
    req[j][over[0]] = alloc[over[0]] - mine[over[0]] + past
    r["node_requests"] = req.reshape(-1)


def _custom_key_pair():
    """`first` opens a machine of `open`; `teamed` names the custom label team=a, which only the second provisioner defines, and opens a machine of that one.  Claimed:
    the first machine ended with `teamed`'s requirement on the key (a later pod added it) -- and, in the second of the pair, is of the template that has the key."""
    its = fake.instance_types(6)
    provs = [fake.provisioner("open", len(its), weight=10), fake.provisioner("teamed", len(its), weight=1, labels={"team": "a"})]
    make = lambda: clause_problem([six_core_pod("first", "2500m"), six_core_pod("teamed", "2400m", {"team": "a"})], provs)

    def edit(r, s, prob, admit):
        j0, j1 = opened_in_order(r, s, prob, 0, 1)
        assert int(r["node_tmpl"][j0]) == 0 and int(r["node_tmpl"][j1]) == 1, r["node_tmpl"]
        k = custom_key(prob, class_of(prob, r, 1))
        assert not (int(prob["tmpl.present"][0]) >> k) & 1 and (int(prob["tmpl.present"][1]) >> k) & 1
        copy_key(r, prob, k, j1, j0)
        assert (int(r["node_present"][j0]) >> k) & 1
        if admit:
            r["node_tmpl"][j0] = 1
        return 1
    return make, edit, "FIT_NEW"


def _does_not_exist_pair():
    """Two pods fill a machine; `without`, which asks for team DoesNotExist, opens the next.  Claimed: the first machine has room for it and ended with team DoesNotExist
    itself -- and, in the second of the pair, without the key."""
    make = lambda: clause_problem([six_core_pod("first", "2500m"), six_core_pod("second", "2500m"),
                                   six_core_pod("without", "2400m", required_affinity=[[Expr("team", "DoesNotExist")]])])

    def edit(r, s, prob, admit):
        j0, j1 = opened_in_order(r, s, prob, 0, 2)
        assert new_node_of(prob, r, 1) == j0
        R, c = prob["R"], class_of(prob, r, 2)
        req = np.asarray(r["node_requests"], dtype=np.int64).reshape(-1, R).copy()
        req[j0] -= prob["cls_requests"][class_of(prob, r, 1) * R:(class_of(prob, r, 1) + 1) * R].astype(np.int64)
        r["node_requests"] = req.reshape(-1)
        k = custom_key(prob, c)
        copy_key(r, prob, k, j1, j0)
        K = prob["K"]
        assert (int(r["node_present"][j0]) >> k) & 1 and not (int(r["node_complement"][j0]) >> k) & 1 and int(np.asarray(r["node_mask"]).reshape(-1, K)[j0, k]) == 0      # DoesNotExist
        if admit:
            a = np.asarray(r["node_present"]).copy()
            a[j0] = int(a[j0]) & ~(1 << k)
            r["node_present"] = a
        return 2
    return make, edit, "FIT_NEW"


def fits_pair(bit="FIT_NEW", filler=None, **late):
    """Two pods fill a machine of the six-core type; `late` opens the next.  Claimed: the first machine's requests are such that with `late` on top the need is one
    milli-unit past the type's allocatable -- and, in the second of the pair, equal to it.  filler, late: what the other passes' pods carry."""
    filler = filler or {}
    make = lambda: clause_problem([six_core_pod("first", "2500m", filler), six_core_pod("second", "2500m", filler), TC._pod("late", cpu="2400m", mem="1Gi", **late)])

    def edit(r, s, prob, admit):
        j0, j1 = opened_in_order(r, s, prob, 0, 2)
        assert new_node_of(prob, r, 1) == j0
        boundary_requests(r, prob, j0, class_of(prob, r, 2), 0 if admit else 1)
        return 2
    return make, edit, bit


def taint_pair(bit="FIT_TEMPLATE", tolerant=None, intolerant=None):
    """The first provisioner taints its machines.  `tolerant` opens a machine of it, `intolerant` one of the second.  Claimed: the target's machine is of the second
    template -- `intolerant` is the target of the first of the pair (a fresh machine of the first template refuses it), `tolerant` of the second.  The pair differs in the
    target pod's toleration, the one thing the clause reads besides the problem's own taints, which no claimed array carries: `intolerant`'s machine is of the second
    template already, so the refusing claimed result is the genuine one and only the admitting one is an edit -- weaker than the other pairs, where both are edits, and
    still enough to catch a dropped or inverted taint clause (the kernels would flag `intolerant` where the reference does not, or miss `tolerant`)."""
    its = fake.instance_types(6)
    provs = [fake.provisioner("tainted", len(its), weight=10, taints=[Taint("dedicated", "x")]), fake.provisioner("open", len(its), weight=1)]
    make = lambda: clause_problem([six_core_pod("tolerant", "3500m", tolerations=[Toleration(key="dedicated", operator="Exists")], **(tolerant or {})),
                                   six_core_pod("intolerant", "3400m", **(intolerant or {}))], provs)

    def edit(r, s, prob, admit):
        j0, j1 = new_node_of(prob, r, 0), new_node_of(prob, r, 1)
        assert j0 != j1 and int(r["node_tmpl"][j0]) == 0 and int(r["node_tmpl"][j1]) == 1 and int(prob["tmpl_taints"][0]) and not int(prob["tmpl_taints"][1]), (r["node_tmpl"], prob["tmpl_taints"])
        target = 0 if admit else 1
        r["node_tmpl"][new_node_of(prob, r, target)] = 1
        return target
    return make, edit, bit


FITS_NAMES = ("Fits: one milli-unit past the allocatable of the only remaining type", "Fits: need == allocatable of the only remaining type")
TAINT_NAMES = ("a template taint the class does not tolerate", "a template taint the class tolerates")
CLAUSE_PAIRS = [("a later pod added a custom key the template lacks", "the same node on a template that has the key", _custom_key_pair),
                ("node final DoesNotExist against class DoesNotExist", "the same node without the key", _does_not_exist_pair),
                FITS_NAMES + (lambda: fits_pair(node_selector=SIX_CORES),), TAINT_NAMES + (taint_pair,)]


def clause_names(pairs):
    return [n + (": admitted" if i else ": not admitted") for refused, admitted, _ in pairs for i, n in enumerate((refused, admitted))]


CLAUSE_NAMES = clause_names(CLAUSE_PAIRS)


def run_clause_pairs(S, pairs, compare, assert_clean, problem_arrays, bits, fit_new_or_template):
    """[(name, True or what differs)], two per pair: the problem solved (at most 8 pods, 3 templates, 6 types, 2 existing nodes) and its genuine result clean; then
    each of the pair's two claimed results audited by the device pass and the reference through `compare` -- bit for bit, counters included -- and the target pod's
    word: none of `fit_new_or_template` where the clause refuses, the pair's bit and nothing else where it admits."""
    report = []
    for (refused, admitted, pair), names in zip(pairs, zip(*[iter(clause_names(pairs))] * 2)):
        make, edit, bit = pair()
        flat = S.FlatProblem(make())
        try:
            flat.solve(decode=False)
            assert flat.dims["P"] <= 8 and flat.dims["M"] <= 3 and flat.dims["T"] <= 6 and flat.dims["E"] <= 2, flat.dims
            assert_clean(S, flat)
            prob = problem_arrays(S, flat)
            for admit, name in zip((False, True), names):
                try:
                    r, s = _claimable(flat.result_arrays()), np.array(flat.pod_seq(), dtype=np.int32)
                    target = edit(r, s, prob, admit)
                    got = compare(S, flat, r, s)[1]
                    word = int(got[target])
                    if admit:
                        ok = True if word == bits[bit] else "pod %d carries %d, expected %s alone: %s" % (target, word, bit, flagged(got))
                    else:
                        ok = True if not word & fit_new_or_template else "pod %d carries %d, expected neither new-node bit: %s" % (target, word, flagged(got))
                except AssertionError as e:
                    ok = "%s" % (e,)
                report.append((name, ok))
        except AssertionError as e:
            report.extend((name, "%s" % (e,)) for name in names)
        flat.close()
    assert [x[0] for x in report] == clause_names(pairs)
    return report


def run_clauses(S):
    return run_clause_pairs(S, CLAUSE_PAIRS, compare, assert_clean, FR.problem_arrays, B, B["FIT_NEW"] | B["FIT_TEMPLATE"])
