"""What tests/test_audit_hostfit.py (on the lane-fibre emulator) and tests/test_audit_hostfit_gpu.py (on the device) share: the comparison of the audit's sixth pass
with its reference (tests/audit_hostfit_ref.py, through tests/audit_harness.py), the hand-made problems -- pods under hostname anti-affinity and hostname spread over existing nodes, new nodes and two
templates, where the reference's first fit is known from how the problem was made --, the tamper matrix, the claimed results with indices out of range and the shapes
at which the kernels take another path.  Every function takes the scheduler module `S` it is to go through (the HIP libraries' or the emulator's)."""
import copy

import numpy as np

import audit_cases as C
import audit_harness as H
from audit_harness import _claimable, flagged
import audit_firstfit_cases as FC
import audit_hostfit_ref as HR
import audit_topo_cases as TC
from karpenter_core_amd import fake
from karpenter_core_amd.model import DO_NOT_SCHEDULE, LABEL_HOSTNAME, ClusterPod, Container, LabelSelector, Pod, PodAffinityTerm, Problem, TopologySpreadConstraint

B = HR.BITS
D = H.PASSES["hostfit"]      # the pass, and its comparison with the reference (tests/audit_harness.py)
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary
HFIT = B["HFIT_EXISTING"] | B["HFIT_NEW"] | B["HFIT_TEMPLATE"]
HISTORICAL_POD = 810      # rr_problem(9013): the pod a stale window flag once gave a machine of its own while a node held by a worker had room


def is_examined(prob, res, seq, p):
    """does the reference examine pod p?  Making it fail SEQ (a commit number out of range) must add one skipped pod"""
    if int(res["pod_node"][p]) < 0:
        return None
    s = np.array(seq, dtype=np.int64)
    before = HR.audit(prob, res, s)[3]
    s[p] = 1 << 30
    return HR.audit(prob, res, s)[3] == before + 1


def class_of(prob, res, p):
    return int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + int(res["pod_stage"][p])])


def to_an_added_node(r, prob, q, like):
    """Edit claimed result `r`: pod q leaves its node for an ADDED new node whose template, requirements, presence masks and options are new node `like`'s and whose
    requests are the template's daemon overhead plus q's own; q's old node, if it is a new node, gives q's requests back -- the fourth pass's matrix's edit."""
    R, K, TW, E = prob["R"], prob["K"], (prob["T"] + 63) // 64, prob["E"]
    c = class_of(prob, r, q)
    req = np.asarray(r["node_requests"], dtype=np.int64).reshape(-1, R).copy()
    mine = prob["cls_requests"][c * R:(c + 1) * R].astype(np.int64)
    tmpl = int(r["node_tmpl"][like])
    added = prob["tmpl_daemon"][tmpl * R:(tmpl + 1) * R].astype(np.int64) + mine
    old = int(r["pod_node"][q]) - E
    if old >= 0:
        req[old] -= mine
    r["node_requests"] = np.concatenate([req, added[None, :]]).reshape(-1)
    for name, width in (("node_tmpl", 1), ("node_types", TW), ("node_requests_present", 1), ("node_present", 1), ("node_complement", 1), ("node_mask", K), ("node_gt", K), ("node_lt", K),
                        ("node_it_state", 1)):
        a = np.asarray(r[name]).reshape(-1, width)
        r[name] = np.concatenate([a, a[like:like + 1]]).reshape(-1)
    r["pod_node"][q] = E + int(r["n_new"])
    r["n_new"] = int(r["n_new"]) + 1


# ---------------------------------------------------------------------------------------------------------------- the historical case: rr_problem(9013)
def historical_case(S, flat):
    """On the CORRECT result of rr_problem(9013) that `flat` holds: pod 810 -- or, had it opened its own node there, the next examined pod of its class by commit number
    that did not -- is claimed as the opener of an added node while the node it joined, opened earlier, has room again.  Returns a dict: the pod, whether it is 810,
    whether the reference examines 810, the flags it got and True or what is wrong."""
    prob, res = HR.problem_arrays(S, flat), flat.result_arrays()
    seq = H.commit_numbers(S, flat, prob)
    E, NS = prob["E"], prob["E"] + int(res["n_new"])
    opened = {}
    for p in range(prob["P"]):
        nd = int(res["pod_node"][p])
        if nd >= E:
            opened[nd] = min(opened.get(nd, 1 << 40), int(seq[p]))
    c = class_of(prob, res, HISTORICAL_POD)
    joiner = lambda p: E <= int(res["pod_node"][p]) < NS and opened[int(res["pod_node"][p])] != int(seq[p])
    pool = sorted((p for p in range(prob["P"]) if class_of(prob, res, p) == c and joiner(p) and seq[p] >= seq[HISTORICAL_POD]), key=lambda p: int(seq[p]))
    out = {"pod_810_examined": is_examined(prob, res, seq, HISTORICAL_POD), "pod_810_node": int(res["pod_node"][HISTORICAL_POD]), "pod_810_opened_it": not joiner(HISTORICAL_POD)}
    if not pool:
        out["ok"] = "no pod of pod 810's class joined a new node"
        return out
    q = pool[0]
    r, s = _claimable(res), np.array(seq, dtype=np.int32)
    to_an_added_node(r, prob, q, int(res["pod_node"][q]) - E)
    out["pod"] = q
    try:
        dev, flags = compare(S, flat, r, s)
    except AssertionError as e:
        out["ok"] = "device and reference differ: %s" % (e,)
        return out
    out["flags"] = int(flags[q])
    out["others_flagged"] = int((flags != 0).sum()) - 1
    first = flat.audit(r)
    out["first_pass"] = {"pods": {k: v for k, v in first["pod_bit_count"].items() if v}, "nodes": {k: v for k, v in first["node_bit_count"].items() if v}}
    out["ok"] = True if int(flags[q]) == B["HFIT_NEW"] else "pod %d carries %d, expected HFIT_NEW" % (q, int(flags[q]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix
TAMPER_NAMES = ["a hostname-spread pod moved to a later existing node", "a placed hostname anti-affinity pod claimed unscheduled",
                "an opener's node re-templated to the later template", "two pods given one commit number"]
PODS = ["ha_a", "ha_b", "nh_a", "nh_b", "plain", "sp_0", "sp_1", "sp_2"]


def tamper_problem() -> Problem:
    """Four roomy existing nodes and two provisioners without limits (`open` before `second`).  ha_a / ha_b (hostname anti-affinity among themselves) go to e0 / e1;
    sp_0 .. sp_2 (self-selecting hostname spread, maxSkew 1) to e0 / e1 / e2; nh_a / nh_b (64 cores each -- no existing node holds one -- and hostname anti-affinity
    among themselves) open a machine of `open` each; `plain` is the fourth pass's pod.  e3 stays empty."""
    its = fake.instance_types(6) + [fake.new_instance_type("huge", {"cpu": "96", "memory": "256Gi", "pods": "200"})]
    provs = [fake.provisioner("open", len(its), weight=10), fake.provisioner("second", len(its), weight=1)]
    nodes = [TC._roomy("e%d" % i, C.Z1) for i in range(4)]
    pods = [TC._pod("ha_a", app="ha", anti_required=TC._anti(LABEL_HOSTNAME, "ha")), TC._pod("ha_b", app="ha", anti_required=TC._anti(LABEL_HOSTNAME, "ha")),
            TC._pod("nh_a", app="nh", cpu="64", anti_required=TC._anti(LABEL_HOSTNAME, "nh")), TC._pod("nh_b", app="nh", cpu="64", anti_required=TC._anti(LABEL_HOSTNAME, "nh")),
            TC._pod("plain")] + [TC._pod("sp_%d" % i, app="sp", spread=[TopologySpreadConstraint(1, LABEL_HOSTNAME, DO_NOT_SCHEDULE, TC._sel("sp"))]) for i in range(3)]
    assert [p.uid for p in pods] == PODS
    return Problem(instance_types=its, provisioners=provs, pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def check_genuine(res, seq):
    pod = {n: i for i, n in enumerate(PODS)}
    where = {n: int(res["pod_node"][i]) for n, i in pod.items()}
    assert res["n_existing"] == 4 and res["n_new"] == 2 and not len(res["unscheduled"]), (res["n_existing"], res["n_new"], where)
    assert [where[n] for n in ("ha_a", "ha_b", "sp_0", "sp_1", "sp_2", "plain")] == [0, 1, 0, 1, 2, 0], where
    assert sorted((where["nh_a"], where["nh_b"])) == [4, 5] and list(res["node_tmpl"]) == [0, 0], (where, res["node_tmpl"])
    assert sorted(int(s) for s in seq) == list(range(len(PODS)))
    return pod


def tampers(res, seq):
    """[(name, edited copy of `res`, edited copy of `seq`, {pod: bits} -- exactly these flags, on exactly these pods)]"""
    pod = check_genuine(res, seq)
    out = []

    def case(name):
        r, s, want = _claimable(res), np.array(seq, dtype=np.int32), {}
        out.append((name, r, s, want))
        return r, s, want
    r, s, want = case(TAMPER_NAMES[0])      # e2, left behind with a count of 0, still takes it
    r["pod_node"][pod["sp_2"]] = 3
    want[pod["sp_2"]] = B["HFIT_EXISTING"]
    r, s, want = case(TAMPER_NAMES[1])      # e1, e2 and e3, both machines (64 of 96 cores taken, no pod of `ha` on them) and a fresh one would all take it
    q = pod["ha_b"]
    r["pod_node"][q] = -1
    s[s > s[q]] -= 1
    s[q] = -1
    r["unscheduled"] = np.array([q], dtype=np.int32)
    want[q] = HFIT
    r, s, want = case(TAMPER_NAMES[2])      # template 0 takes nh_a on a fresh machine: it cannot have opened one of template 1
    r["node_tmpl"][int(res["pod_node"][pod["nh_a"]]) - 4] = 1
    want[pod["nh_a"]] = B["HFIT_TEMPLATE"]
    r, s, want = case(TAMPER_NAMES[3])
    s[pod["sp_1"]] = s[pod["sp_0"]]
    want[pod["sp_0"]] = want[pod["sp_1"]] = B["SEQ"]
    assert [o[0] for o in out] == TAMPER_NAMES
    return out


def run_tamper_matrix(S):
    """Solve `tamper_problem`, audit the genuine result (clean; the fourth pass examines `plain` alone, this one the other seven) and every edit through the claimed form,
    where the first pass must find nothing in the first two; returns [(name, True or what differs)]."""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    fourth = flat.audit_firstfit()
    assert flat.dims["M"] == 2 and dev["checked"]["PODS"] == 7 and dev["skipped_pods"] == 1 and fourth["checked"]["PODS"] == 1 and dev["admitting_pairs"] > 0 and dev["checked"]["TESTS"] > 0, (dev, fourth)
    res, seq = flat.result_arrays(), flat.pod_seq()
    report = []
    for name, claimed, s, want in tampers(res, seq):
        try:
            d, flags = compare(S, flat, claimed, s)
            ok = True if flagged(d["pod_flags"]) == want else "flags %s, expected %s" % (flagged(d["pod_flags"]), want)
        except AssertionError as e:
            ok = "device and reference differ: %s" % (e,)
        if ok is True and name in TAMPER_NAMES[:2]:
            first = flat.audit(claimed)
            if first["n_pods_flagged"] or first["n_nodes_flagged"]:
                ok = "the first pass flags the edit: %s %s" % (first["pod_bit_count"], first["node_bit_count"])
        report.append((name, ok))
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- claimed results with indices out of range
RANGE_NAMES = ["pod_node far out of range", "pod_node == E + n_new", "pod_stage out of range", "node_tmpl out of range", "pod_seq out of range", "every index out of range at once"]


def run_range_cases(S):
    """Out-of-range pod_node, pod_stage, node_tmpl and pod_seq in a claimed result of `tamper_problem`: device and reference agree -- flags or skips -- and the pods the
    edit does not touch keep clean words.  (An index that addressed memory past a table would not agree with a reference that never reads it.)"""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    res, seq = flat.result_arrays(), flat.pod_seq()
    pod = check_genuine(res, seq)
    big, small = 2 ** 31 - 1, -2 ** 31

    def edit(name, r, s):
        if name == RANGE_NAMES[0]:
            r["pod_node"][pod["sp_0"]], r["pod_node"][pod["ha_a"]], r["pod_node"][pod["nh_a"]] = big, small, -7
        elif name == RANGE_NAMES[1]:
            r["pod_node"][pod["sp_1"]] = 4 + int(r["n_new"])
        elif name == RANGE_NAMES[2]:
            r["pod_stage"][pod["sp_0"]], r["pod_stage"][pod["ha_b"]], r["pod_stage"][pod["nh_b"]] = big, small, 1
        elif name == RANGE_NAMES[3]:
            r["node_tmpl"][0], r["node_tmpl"][1] = big, small
        elif name == RANGE_NAMES[4]:
            s[pod["sp_0"]], s[pod["ha_a"]], s[pod["nh_a"]], s[pod["plain"]] = big, small, len(PODS), -1
        else:
            for n in RANGE_NAMES[:5]:
                edit(n, r, s)
    report = []
    for name in RANGE_NAMES:
        r, s = _claimable(res), np.array(seq, dtype=np.int32)
        edit(name, r, s)
        try:
            compare(S, flat, r, s)
            ok = True
        except AssertionError as e:
            ok = "device and reference differ: %s" % (e,)
        report.append((name, ok))
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- shapes where the kernels take another path
def _spread(skew, app):
    return [TopologySpreadConstraint(skew, LABEL_HOSTNAME, DO_NOT_SCHEDULE, TC._sel(app))]


def _problem(pods, nodes=(), cluster_pods=(), types=4, provs=None):
    its = fake.instance_types(types)
    return Problem(instance_types=its, provisioners=provs or [fake.provisioner("open", len(its))], pods=list(pods), nodes=list(nodes), cluster_pods=list(cluster_pods),
                   extra_well_known=fake.EXTRA_WELL_KNOWN)


def many_groups(n: int) -> Problem:
    """n pods under n different self-selecting hostname spreads: n eligible groups, every pod on e0."""
    return _problem([TC._pod("g%03d" % i, app="g%03d" % i, spread=_spread(1, "g%03d" % i)) for i in range(n)], [TC._roomy("e0", C.Z1), TC._roomy("e1", C.Z2)])


def crowded_class(k: int = 1) -> Problem:
    """`target` owns a hostname spread and a hostname anti-affinity term and is selected by the anti-affinity terms of k `wary` pods, each over a label of its own:
    its class is constrained by 2 + k groups (own spread + own anti-affinity + k inverse); the flattening refuses a pod under more than three hostname-keyed groups.  The
    wary pods fill e0 .. e(k-1); the target takes the next node."""
    labels = {"app": "target"}
    labels.update({"l%d" % i: "x" for i in range(k)})
    target = Pod(uid="target", labels=labels, containers=[Container(requests={"cpu": "100m", "memory": "64Mi"})], spread=_spread(1, "target"), anti_required=TC._anti(LABEL_HOSTNAME, "other"))
    wary = [TC._pod("wary-%d" % i, cpu="200m", anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"l%d" % i: "x"}))]) for i in range(k)]
    return _problem(wary + [target], [TC._roomy("e%d" % i, C.Z1) for i in range(3)])


def spread_pods(n: int, existing: bool) -> Problem:
    """n pods under one self-selecting hostname spread with maxSkew n: one node takes them all -- e0, or a new machine."""
    return _problem([TC._pod("s%d" % i, app="s", spread=_spread(max(1, n), "s")) for i in range(n)], [TC._roomy("e0", C.Z1)] if existing else [])


def one_node_admits(E: int, at: int) -> Problem:
    """E roomy existing nodes; every node but `at` holds one pod of app `m` (bound there by a hostname selector); `wary` has hostname anti-affinity against `m`:
    the count alone decides that node `at` is the only one that takes it."""
    nodes = [TC._roomy("e%03d" % i, C.Z1) for i in range(E)]
    pods = [TC._pod("m%03d" % i, app="m", cpu="200m", node_selector={LABEL_HOSTNAME: "e%03d" % i}) for i in range(E) if i != at]
    return _problem(pods + [TC._pod("wary", anti_required=TC._anti(LABEL_HOSTNAME, "m"))], nodes)


def one_new_node_admits(n: int = 65) -> Problem:
    """n pods of 3 cores with hostname anti-affinity among themselves open n machines; all but the largest (the first in the queue) also carry `mark`.  `wary`, with
    hostname anti-affinity against `mark`, is taken by the first-opened machine alone."""
    def big(i):
        labels = {"app": "big"}
        if i:
            labels["mark"] = "y"
        return Pod(uid="big-%03d" % i, labels=labels, containers=[Container(requests={"cpu": "3100m" if i == 0 else "3000m", "memory": "64Mi"})], anti_required=TC._anti(LABEL_HOSTNAME, "big"))
    wary = TC._pod("wary", anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"mark": "y"}))])
    return _problem([big(i) for i in range(n)] + [wary], types=6)


def one_type_fits(T: int) -> Problem:
    """The ladder of T types -- type i has i + 1 cores -- and one pod under a hostname spread that only the largest holds."""
    return _problem([TC._pod("wide", app="w", cpu="%dm" % (T * 1000 - 500), mem="64Mi", spread=_spread(1, "w"))], types=T)


def skew_problem(skew: int, self_sel: bool, held: int) -> Problem:
    """e0 holds `held` pods of app `m` (bound there by a hostname selector, larger: earlier in the queue); `s` owns a hostname spread over `m` with maxSkew `skew` and
    carries the label itself or not.  It fits e0 iff held + self <= skew; else it goes to e1."""
    pods = [TC._pod("m%d" % i, app="m", cpu="200m", node_selector={LABEL_HOSTNAME: "e0"}) for i in range(held)]
    return _problem(pods + [TC._pod("s", app="m" if self_sel else "other", spread=_spread(skew, "m"))], [TC._roomy("e0", C.Z1), TC._roomy("e1", C.Z1)])


def init_problem(count: int) -> Problem:
    """e0 starts with `count` pods of app `m` already bound in the cluster (countDomains: init = count); `wary`, with hostname anti-affinity against `m`, takes e0 iff 0."""
    cps = [ClusterPod(uid="bound-%d" % i, namespace="default", node_name="e0", labels={"app": "m"}) for i in range(count)]
    return _problem([TC._pod("wary", anti_required=TC._anti(LABEL_HOSTNAME, "m"))], [TC._roomy("e0", C.Z1), TC._roomy("e1", C.Z1)], cps)


def many_classes(n: int) -> Problem:
    """n pods of n different requests under one self-selecting hostname spread with maxSkew n: n used classes, all on e0."""
    return _problem([TC._pod("c%03d" % i, app="c", cpu="%dm" % (i + 1), spread=_spread(n, "c")) for i in range(n)], [TC._roomy("e0", C.Z1), TC._roomy("e1", C.Z2)])


def crowded_node(n: int) -> Problem:
    """n + 1 pods of one millicore under one self-selecting hostname spread with maxSkew n: e0 takes n, the last goes to e1 -- which is right only if e0's count is n
    to the unit."""
    return _problem([TC._pod("m%04d" % i, app="m", cpu="1m", mem="1Mi", spread=_spread(n, "m")) for i in range(n + 1)], [TC._roomy("e0", C.Z1), TC._roomy("e1", C.Z2)])


def wide_problem() -> Problem:
    from karpenter_core_amd import workloads as W
    pr = copy.copy(W.wide_catalogue(names=12, pods=60, types=10, existing=4, seed=3, dense=True))
    pr.pods = list(pr.pods) + [TC._pod("zz-spread-%d" % i, app="zz", cpu="10m", mem="8Mi", spread=_spread(1, "zz")) for i in range(3)]
    return pr


SKEWS = [(skew, self_sel) for skew in (1, 2) for self_sel in (False, True)]
NODE_SHAPES = [(65, 0), (65, 63), (257, 0), (257, 255)]
TYPE_SHAPES = [(1, 0), (65, 64)]
SHAPE_NAMES = ["%d eligible groups" % n for n in (1, 64, 65)] + ["a class under 3 groups, the most a problem may hold: own spread, own anti-affinity, one inverse", "E = 0", "n_new = 0", "P = 1"] + \
              ["E = %d: the only admitting node at index %d" % ns for ns in NODE_SHAPES] + ["65 new nodes: only the first-opened admits"] + \
              ["T = %d: the only admitting type at bit %d" % ts for ts in TYPE_SHAPES] + \
              ["maxSkew %d, %s: at the boundary and one past it" % (k, "self" if s else "not self") for k, s in SKEWS] + ["init 0 and 1", "257 used classes", "a node with 1 100 pods",
               "12 resource names", "two templates"]


def run_shapes(S):
    """[(name, True or what differs)] -- each shape solved (clean by device and reference) and, where it says so, one claimed edit."""
    report = []

    def solved(make, body):
        flat = S.FlatProblem(make())
        try:
            flat.solve(decode=False)
            dev = assert_clean(S, flat)
            return body(flat, dev)
        finally:
            flat.close()

    def shape(name, make, body):
        try:
            ok = solved(make, body)
        except Exception as e:
            ok = "%s: %s" % (type(e).__name__, e)
        report.append((name, ok))

    def claim(flat, edit):
        res, seq = _claimable(flat.result_arrays()), np.array(flat.pod_seq(), dtype=np.int32)
        edit(res, seq)
        dev, flags = compare(S, flat, res, seq)
        return flagged(flags)

    def unschedule(p):
        def edit(r, s):
            s[s > s[p]] -= 1
            r["pod_node"][p], s[p], r["unscheduled"] = -1, -1, np.array([p], dtype=np.int32)
        return edit

    def move(p, to):
        def edit(r, s):
            r["pod_node"][p] = to
        return edit

    def groups(n):
        def body(flat, dev):
            assert dev["eligible_groups"] == n and dev["skipped_groups"] == 0 and dev["checked"]["PODS"] == n and dev["checked"]["TESTS"] == dev["checked"]["PAIRS"], dev
            got = claim(flat, move(n - 1, 1))      # the last group's slot: e0, without that pod, takes it
            assert got == {n - 1: B["HFIT_EXISTING"]}, got
            return True
        return body
    for n, name in zip((1, 64, 65), SHAPE_NAMES):
        shape(name, lambda n=n: many_groups(n), groups(n))

    def crowded(flat, dev):
        prob, res = HR.problem_arrays(S, flat), flat.result_arrays()
        c = class_of(prob, res, 1)
        n = int(prob["cls_own_off"][c + 1]) - int(prob["cls_own_off"][c]) + int(prob["cls_isel_off"][c + 1]) - int(prob["cls_isel_off"][c])
        assert n == 3 and dev["checked"]["PODS"] == 2 and dev["skipped_groups"] == 0 and [int(x) for x in res["pod_node"]] == [0, 1], (n, dev, res["pod_node"])
        got = claim(flat, unschedule(1))      # three count tests per pair; e1, e2 and a fresh machine take the target
        assert got == {1: B["HFIT_EXISTING"] | B["HFIT_TEMPLATE"]}, got
        return True
    shape(SHAPE_NAMES[3], crowded_class, crowded)
    shape("E = 0", lambda: spread_pods(3, False), lambda flat, dev: True if flat.dims["E"] == 0 and dev["n_new"] == 1 and dev["checked"] == {"SEQ": 3, "PODS": 3, "PAIRS": 2, "TESTS": 2} else str(dev))
    shape("n_new = 0", lambda: spread_pods(3, True), lambda flat, dev: True if dev["n_new"] == 0 and dev["checked"] == {"SEQ": 3, "PODS": 3, "PAIRS": 2, "TESTS": 2} and dev["admitting_pairs"] == 1 else str(dev))
    shape("P = 1", lambda: spread_pods(1, False), lambda flat, dev: True if flat.dims["P"] == 1 and dev["checked"] == {"SEQ": 1, "PODS": 1, "PAIRS": 2, "TESTS": 2} else str(dev))

    def only_node(E, at):
        def body(flat, dev):
            res = flat.result_arrays()
            wary = E - 1
            # (the pods of `m` are examined too: wary's term selects them, an inverse group constrains them -- each is admitted by the node it names alone)
            assert flat.dims["E"] == E and int(res["pod_node"][wary]) == at and dev["checked"]["PODS"] == E and dev["admitting_pairs"] == E + 1, (res["pod_node"][wary], dev["checked"], dev["admitting_pairs"])
            got = claim(flat, move(wary, E - 1))      # the minimum over the existing nodes crosses lanes, waves and workgroups
            assert got == {wary: B["HFIT_EXISTING"]}, got
            return True
        return body
    for (E, at), name in zip(NODE_SHAPES, SHAPE_NAMES[7:11]):
        shape(name, lambda E=E, at=at: one_node_admits(E, at), only_node(E, at))

    def only_new_node(flat, dev):
        prob, res, seq = HR.problem_arrays(S, flat), flat.result_arrays(), flat.pod_seq()
        wary = 65
        assert res["n_new"] == 65 and int(res["pod_node"][wary]) == int(res["pod_node"][0]) and int(seq[0]) == 0 and dev["checked"]["PODS"] == 66, (res["n_new"], res["pod_node"][wary], res["pod_node"][0], dev)

        def edit(r, s):
            to_an_added_node(r, prob, wary, int(res["pod_node"][wary]) - prob["E"])
        got = claim(flat, edit)      # the first-opened machine has room again: the minimum of open() over 65 (+ 1) new nodes finds it
        assert got == {wary: B["HFIT_NEW"]}, got
        return True
    shape(SHAPE_NAMES[11], one_new_node_admits, only_new_node)

    def last_type(T, bit):
        def body(flat, dev):
            res = flat.result_arrays()
            words = np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, (T + 63) // 64)
            assert flat.dims["T"] == T and res["n_new"] == 1 and [int(w) for w in words[0]] == [(1 << (bit % 64)) if i == bit // 64 else 0 for i in range(words.shape[1])], (flat.dims, words)
            assert dev["checked"] == {"SEQ": 1, "PODS": 1, "PAIRS": 2, "TESTS": 2} and dev["admitting_pairs"] == 1, dev
            got = claim(flat, unschedule(0))      # the walk over the types must reach the one bit to say so
            assert got == {0: B["HFIT_TEMPLATE"]}, got
            return True
        return body
    for (T, bit), name in zip(TYPE_SHAPES, SHAPE_NAMES[12:14]):
        shape(name, lambda T=T: one_type_fits(T), last_type(T, bit))

    def skews(skew, self_sel):
        def run():
            at = skew - (1 if self_sel else 0)      # the most e0 may hold for `s` to fit

            def boundary(flat, dev):
                assert int(flat.result_arrays()["pod_node"][at]) == 0 and dev["checked"]["PODS"] == 1, (flat.result_arrays()["pod_node"], dev)
                got = claim(flat, move(at, 1))      # e0 at the boundary still takes it
                assert got == {at: B["HFIT_EXISTING"]}, got
                return True

            def past(flat, dev):
                assert int(flat.result_arrays()["pod_node"][at + 1]) == 1 and dev["checked"]["PODS"] == 1 and dev["admitting_pairs"] == (2 if 2 * self_sel <= skew else 1), (flat.result_arrays()["pod_node"], dev)      # a fresh machine, and e1 if it takes a second such pod; not e0
                return True
            return solved(lambda: skew_problem(skew, self_sel, at), boundary) and solved(lambda: skew_problem(skew, self_sel, at + 1), past)
        return run
    for (skew, self_sel), name in zip(SKEWS, SHAPE_NAMES[14:18]):
        try:
            ok = skews(skew, self_sel)()
        except AssertionError as e:
            ok = "%s" % (e,)
        report.append((name, ok))

    def inits():
        def zero(flat, dev):
            assert int(flat.result_arrays()["pod_node"][0]) == 0 and dev["admitting_pairs"] == 3, (flat.result_arrays()["pod_node"], dev)      # e0 (it holds the pod itself, which records nothing of the group), e1 and a fresh machine
            return True

        def one(flat, dev):
            assert int(flat.result_arrays()["pod_node"][0]) == 1 and dev["checked"]["PAIRS"] == 3 and dev["admitting_pairs"] == 2, (flat.result_arrays()["pod_node"], dev)      # e1 and a fresh machine: e0's init of 1 refuses
            return True
        return solved(lambda: init_problem(0), zero) and solved(lambda: init_problem(1), one)
    try:
        ok = inits()
    except AssertionError as e:
        ok = "%s" % (e,)
    report.append(("init 0 and 1", ok))

    def classes_257(flat, dev):
        assert flat.dims["C"] >= 257 and dev["checked"] == {"SEQ": 257, "PODS": 257, "PAIRS": 257 * 3, "TESTS": 257 * 3} and dev["admitting_pairs"] == 257 * 2 and dev["n_new"] == 0, dev      # (e0, at maxSkew, refuses)
        got = claim(flat, move(256, 1))      # the class past the scan tile finds its own row of the first_* tables: e0, without the pod, takes it
        assert got == {256: B["HFIT_EXISTING"]}, got
        return True
    shape("257 used classes", lambda: many_classes(257), classes_257)

    def crowd(flat, dev):
        where = np.asarray(flat.result_arrays()["pod_node"])
        assert int((where == 0).sum()) == 1100 and int((where == 1).sum()) == 1 and dev["checked"] == {"SEQ": 1101, "PODS": 1101, "PAIRS": 3, "TESTS": 3} and dev["admitting_pairs"] == 2, (dev, (where == 0).sum())
        return True
    shape("a node with 1 100 pods", lambda: crowded_node(1100), crowd)
    shape("12 resource names", wide_problem, lambda flat, dev: True if flat.dims["R"] == 12 and dev["checked"]["PODS"] >= 3 and dev["admitting_pairs"] > 0 else str((flat.dims, dev)))
    shape("two templates", tamper_problem, lambda flat, dev: True if flat.dims["M"] == 2 and dev["checked"]["PAIRS"] == 3 * (4 + 2 + 2) else str(dev))
    assert [r[0] for r in report] == SHAPE_NAMES, [r[0] for r in report]
    return report


# ---------------------------------------------------------------------------------------------------------------- two clauses of the new-node predicate, through this pass's kernels
def _alone(app):
    """hostname anti-affinity against a label the pod alone carries: every count is 0, the new-node predicate decides"""
    return {"app": app, "anti_required": TC._anti(LABEL_HOSTNAME, app)}


CLAUSE_PAIRS = [FC.FITS_NAMES + (lambda: FC.fits_pair("HFIT_NEW", node_selector=FC.SIX_CORES, **_alone("late")),),
                FC.TAINT_NAMES + (lambda: FC.taint_pair("HFIT_TEMPLATE", _alone("tolerant"), _alone("intolerant")),)]
CLAUSE_NAMES = FC.clause_names(CLAUSE_PAIRS)


def run_clauses(S):
    """tests/audit_firstfit_cases.py's Fits pair and taint pair on classes under hostname anti-affinity: [(name, True or what differs)]"""
    return FC.run_clause_pairs(S, CLAUSE_PAIRS, compare, assert_clean, HR.problem_arrays, B, B["HFIT_NEW"] | B["HFIT_TEMPLATE"])
