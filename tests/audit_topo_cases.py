"""What tests/test_audit_topology.py (on the lane-fibre emulator) and tests/test_audit_topology_gpu.py (on the device) share: the comparison of the audit's second
pass with its reference (tests/audit_topo_ref.py, through tests/audit_harness.py), the hand-made problems -- leaders and followers, the tamper matrix's cluster, the shapes at which the kernels take
another path --, and the tamper matrix: one minimal edit of a genuine result or of its commit numbers per rule and direction, with the pods the edit must flag known
from how the problem was made.  Every function takes the scheduler module `S` it is to go through (the HIP libraries' or the emulator's)."""
import copy

import numpy as np

import audit_cases as C
import audit_harness as H
import audit_topo_ref as TR
from karpenter_core_amd import fake
from karpenter_core_amd.model import (DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_ZONE, Container, Expr, LabelSelector, Pod, PodAffinityTerm, Problem, TopologySpreadConstraint)

Z1, Z2, Z3 = C.Z1, C.Z2, C.Z3
B = TR.BITS
D = H.PASSES["topology"]      # the pass, and its comparison with the reference (tests/audit_harness.py)
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary


# ---------------------------------------------------------------------------------------------------------------- hand-made problems
def _pod(uid, app=None, cpu="100m", mem="64Mi", **kw):
    return Pod(uid=uid, labels={"app": app} if app else {}, containers=[Container(requests={"cpu": cpu, "memory": mem})], **kw)


def _sel(app):
    return LabelSelector({"app": app})


def _anti(key, app):
    return [PodAffinityTerm(key, _sel(app))]


def leaders_and_followers() -> Problem:
    """A leader deployment and followers with REQUIRED affinity to it, not self-selecting: on the zone and on the hostname.  No existing node: the leaders open machines,
    the followers -- first in the queue by uid, refused until a leader is placed -- join them.  Exercises the AFFINITY rule, which the generators' self-selecting
    affinity pods (workloads.affinity_pod with equal labels apart) leave to chance."""
    its = fake.instance_types(6)
    pods = [_pod("lead-%d" % i, app="lead", cpu="900m", node_selector={LABEL_ZONE: Z2}) for i in range(3)]
    pods += [_pod("fol-h-%d" % i, cpu="200m", affinity_required=[PodAffinityTerm(LABEL_HOSTNAME, _sel("lead"))]) for i in range(4)]
    pods += [_pod("fol-z-%d" % i, cpu="3", affinity_required=[PodAffinityTerm(LABEL_ZONE, _sel("lead"))]) for i in range(4)]
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=pods, nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def _roomy(name, zone, **labels):
    n = C._node(name, zone, "40")
    n.available = {"cpu": "40", "memory": "64Gi", "pods": "2000"}
    n.labels.update(labels)
    return n


PODS = ["fol_h", "fol_z", "ha_a", "ha_b", "lead", "nh_a", "nh_b", "nz_a", "nz_b", "plain_a", "plain_b", "sp_0", "sp_1", "sp_2", "za_a", "za_b"]
E0, E1, E2, E3 = 0, 1, 2, 3


def tamper_problem() -> Problem:
    """Four roomy existing nodes -- e0 and e1 in zone 1, e2 in zone 2, e3 in zone 3 -- and an open provisioner.  Where the reference puts the pods (first fit over the
    existing nodes in order): ha_a / ha_b (hostname anti-affinity among themselves) on e0 / e1; za_a / za_b (zone anti-affinity among themselves) on e0 / e2; lead on
    e0, fol_h (hostname affinity to lead) and fol_z (zone affinity to lead), both ahead of lead in the queue and refused until it is placed, on e0; sp_0 .. sp_2
    (self-selecting hostname spread, maxSkew 1) on e0 / e1 / e2; plain_a / plain_b on e0.  nh_a / nh_b (64 cores each: no existing node holds them; hostname
    anti-affinity among themselves) and nz_a / nz_b (the same with zone anti-affinity; nz_a names zone 3 -- a machine open to every zone would record them all,
    topology.go:125-127, and leave nz_b none) on four new nodes."""
    its = fake.instance_types(6) + [fake.new_instance_type("huge", {"cpu": "96", "memory": "256Gi", "pods": "200"})]
    nodes = [_roomy("e0", Z1), _roomy("e1", Z1), _roomy("e2", Z2), _roomy("e3", Z3)]
    pods = [_pod("fol_h", affinity_required=[PodAffinityTerm(LABEL_HOSTNAME, _sel("lead"))]), _pod("fol_z", affinity_required=[PodAffinityTerm(LABEL_ZONE, _sel("lead"))]),
            _pod("ha_a", app="ha", anti_required=_anti(LABEL_HOSTNAME, "ha")), _pod("ha_b", app="ha", anti_required=_anti(LABEL_HOSTNAME, "ha")),
            _pod("lead", app="lead"),
            _pod("nh_a", app="nh", cpu="64", anti_required=_anti(LABEL_HOSTNAME, "nh")), _pod("nh_b", app="nh", cpu="64", anti_required=_anti(LABEL_HOSTNAME, "nh")),
            _pod("nz_a", app="nz", cpu="64", anti_required=_anti(LABEL_ZONE, "nz"), node_selector={LABEL_ZONE: Z3}), _pod("nz_b", app="nz", cpu="64", anti_required=_anti(LABEL_ZONE, "nz")),
            _pod("plain_a"), _pod("plain_b")] + \
           [_pod("sp_%d" % i, app="sp", spread=[TopologySpreadConstraint(1, LABEL_HOSTNAME, DO_NOT_SCHEDULE, _sel("sp"))]) for i in range(3)] + \
           [_pod("za_a", app="za", anti_required=_anti(LABEL_ZONE, "za")), _pod("za_b", app="za", anti_required=_anti(LABEL_ZONE, "za"))]
    assert [p.uid for p in pods] == PODS
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def check_genuine(res: dict, seq) -> dict:
    """The genuine result is the one `tamper_problem` describes; returns pod name -> index."""
    pod = {n: i for i, n in enumerate(PODS)}
    where = {n: int(res["pod_node"][i]) for n, i in pod.items()}
    assert res["n_existing"] == 4 and res["n_new"] == 4 and not len(res["unscheduled"]), (res["n_existing"], res["n_new"], where)
    assert [where[n] for n in ("ha_a", "ha_b", "za_a", "za_b", "lead", "fol_h", "fol_z", "sp_0", "sp_1", "sp_2", "plain_a", "plain_b")] == [E0, E1, E0, E2, E0, E0, E0, E0, E1, E2, E0, E0], where
    assert len({where[n] for n in ("nh_a", "nh_b", "nz_a", "nz_b")}) == 4 and min(where[n] for n in ("nh_a", "nh_b", "nz_a", "nz_b")) >= 4, where
    assert sorted(int(s) for s in seq) == list(range(len(PODS)))
    assert seq[pod["lead"]] < seq[pod["fol_h"]] and seq[pod["lead"]] < seq[pod["fol_z"]]
    return pod


TAMPER_NAMES = ["a pod moved onto the node of a hostname-anti-affine peer", "the same pair with their commit numbers swapped", "the same on a new node",
                "a pod moved into the zone of a zone-anti-affine peer on another node", "the same on a new node that spans the peer's zone",
                "a hostname follower moved to a node without its leader", "a zone follower moved to a zone without its leader", "a follower given a commit number below its leader's",
                "one owner too many on a node of a hostname spread", "two pods given one commit number", "a commit number past the placed pods"]


def tampers(res: dict, seq):
    """[(name, edited copy of `res`, edited copy of `seq`, {pod index: bits})]: one minimal edit per rule and direction; the flags it must raise -- exactly those, on exactly
    those pods -- follow from how `tamper_problem` was made and from the commit numbers."""
    pod = check_genuine(res, seq)
    out = []

    def case(name):
        r, s = copy.deepcopy({k: v for k, v in res.items() if k != "key_value"}), np.array(seq, dtype=np.int32)
        want = {}
        out.append((name, r, s, want))
        return r, s, want
    later = lambda s, a, b: pod[a] if s[pod[a]] > s[pod[b]] else pod[b]
    r, s, want = case(TAMPER_NAMES[0])
    r["pod_node"][pod["ha_b"]] = E0
    want[later(s, "ha_a", "ha_b")] = B["ANTI_AFFINITY"]
    r, s, want = case(TAMPER_NAMES[1])
    r["pod_node"][pod["ha_b"]] = E0
    was = later(s, "ha_a", "ha_b")
    s[pod["ha_a"]], s[pod["ha_b"]] = s[pod["ha_b"]], s[pod["ha_a"]]
    want[later(s, "ha_a", "ha_b")] = B["ANTI_AFFINITY"]
    assert later(s, "ha_a", "ha_b") != was
    r, s, want = case(TAMPER_NAMES[2])
    r["pod_node"][pod["nh_b"]] = r["pod_node"][pod["nh_a"]]
    want[later(s, "nh_a", "nh_b")] = B["ANTI_AFFINITY"]
    r, s, want = case(TAMPER_NAMES[3])
    r["pod_node"][pod["za_b"]] = E1      # zone 1, where za_a is -- on e0
    want[later(s, "za_a", "za_b")] = B["ANTI_AFFINITY"]
    r, s, want = case(TAMPER_NAMES[4])
    r["pod_node"][pod["nz_b"]] = r["pod_node"][pod["nh_a"]]      # a machine of every zone the provisioner offers: nz_a's among them
    want[later(s, "nz_a", "nz_b")] = B["ANTI_AFFINITY"]
    r, s, want = case(TAMPER_NAMES[5])
    r["pod_node"][pod["fol_h"]] = E1      # the leader's zone, not its node
    want[pod["fol_h"]] = B["AFFINITY"]
    r, s, want = case(TAMPER_NAMES[6])
    r["pod_node"][pod["fol_z"]] = E2
    want[pod["fol_z"]] = B["AFFINITY"]
    r, s, want = case(TAMPER_NAMES[7])
    s[pod["fol_h"]], s[pod["lead"]] = s[pod["lead"]], s[pod["fol_h"]]
    for f in ("fol_h", "fol_z"):
        if s[pod[f]] < s[pod["lead"]]:
            want[pod[f]] = B["AFFINITY"]
    assert pod["fol_h"] in want
    r, s, want = case(TAMPER_NAMES[8])
    r["pod_node"][pod["sp_1"]] = E0
    want[later(s, "sp_0", "sp_1")] = B["HOSTNAME_SPREAD"]
    r, s, want = case(TAMPER_NAMES[9])
    s[pod["plain_b"]] = s[pod["plain_a"]]
    want[pod["plain_a"]] = want[pod["plain_b"]] = B["SEQ"]
    r, s, want = case(TAMPER_NAMES[10])
    s[pod["plain_b"]] = len(PODS)
    want[pod["plain_b"]] = B["SEQ"]
    assert [o[0] for o in out] == TAMPER_NAMES
    return out


def run_tamper_matrix(S):
    """Solve `tamper_problem`, audit the genuine result (clean, every rule evaluated) and every edit through the claimed form; returns [(name, True or what differs)]."""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    assert all(v > 0 for v in dev["checked"].values()), dev["checked"]
    res, seq = flat.result_arrays(), flat.pod_seq()
    report = []
    for name, claimed, s, want in tampers(res, seq):
        want_f = np.zeros(len(PODS), dtype=np.uint32)
        for i, b in want.items():
            want_f[i] = b
        try:
            dev, flags, _ = compare(S, flat, claimed, s)
            report.append((name, True if np.array_equal(dev["pod_flags"], want_f) else "flags %s, expected %s" % ({int(i): int(dev["pod_flags"][i]) for i in np.nonzero(dev["pod_flags"])[0]}, want)))
        except AssertionError as e:
            report.append((name, "device and reference differ: %s" % (e,)))
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- shapes where the kernels take another path
def crowded(extra: int = 0) -> Problem:
    """1 100 (+ extra) tiny pods under a self-selecting hostname spread with maxSkew 1 100 and one existing node: the node's list crosses the wave's stride (64) and
    the LDS tile (256) several times.  The node takes 1 100; one more goes to a new node."""
    its = fake.instance_types(4)
    node = _roomy("crowd", Z1)
    spread = [TopologySpreadConstraint(1100, LABEL_HOSTNAME, DO_NOT_SCHEDULE, _sel("tiny"))]
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=[_pod("tiny-%04d" % i, app="tiny", cpu="1m", mem="1Mi", spread=spread) for i in range(1100 + extra)],
                   nodes=[node], extra_well_known=fake.EXTRA_WELL_KNOWN)


RACK = "example.com/rack"


def racks() -> Problem:
    """A topology key with 64 values: 65 existing nodes, node i in rack min(i, 63) -- the last two share the rack of value id 63 -- and two pods with anti-affinity among
    themselves over the rack, pinned by hostname to nodes 62 and 63."""
    its = fake.instance_types(4)
    nodes = [_roomy("n%02d" % i, Z1, **{RACK: "rack-%02d" % min(i, 63)}) for i in range(65)]
    pods = [_pod("rk_a", app="rk", anti_required=_anti(RACK, "rk"), node_selector={LABEL_HOSTNAME: "n63"}), _pod("rk_b", app="rk", anti_required=_anti(RACK, "rk"), node_selector={LABEL_HOSTNAME: "n62"})]
    prov = fake.provisioner("open", len(its), requirements=[Expr(RACK, "In", ["rack-%02d" % i for i in range(64)])])      # (the racks are domains because the provisioner names them)
    return Problem(instance_types=its, provisioners=[prov], pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def many_groups(n: int = 24) -> Problem:
    """One pod with n required anti-affinity terms over the zone, against n different labels, and one pod carrying the last label, pinned to zone 1: the first lands in
    another zone."""
    its = fake.instance_types(4)
    nodes = [_roomy("e0", Z1), _roomy("e1", Z2)]
    pods = [_pod("target", app="t%d" % (n - 1), node_selector={LABEL_ZONE: Z1}, cpu="200m"),
            _pod("wary", cpu="100m", anti_required=[PodAffinityTerm(LABEL_ZONE, _sel("t%d" % i)) for i in range(n)])]
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def plain(pods: int = 1, existing: bool = False) -> Problem:
    """No topology group at all: G == 0."""
    its = fake.instance_types(4)
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=[_pod("p%d" % i) for i in range(pods)], nodes=[_roomy("e0", Z1)] if existing else [],
                   extra_well_known=fake.EXTRA_WELL_KNOWN)


SHAPE_TAMPER_NAMES = ["a key of 64 values: the violation in value id 63", "24 groups: the violation in the last of them"]


def _claim(S, flat, edit, want_bits, want_pods):
    """Audit the genuine result of `flat` (clean), then the result after `edit(res, seq, prob)`; True, or what differs from `want_bits` on `want_pods(res, seq)`."""
    assert_clean(S, flat)
    res, seq, prob = flat.result_arrays(), flat.pod_seq(), TR.problem_arrays(S, flat)
    res = {k: v for k, v in res.items() if k != "key_value"}
    edit(res, seq, prob)
    want = np.zeros(prob["P"], dtype=np.uint32)
    for p in want_pods(res, seq):
        want[p] = want_bits
    try:
        dev, flags, _ = compare(S, flat, res, seq)
    except AssertionError as e:
        return "device and reference differ: %s" % (e,)
    return True if np.array_equal(dev["pod_flags"], want) else "flags %s" % ({int(i): int(dev["pod_flags"][i]) for i in np.nonzero(dev["pod_flags"])[0]},)


def run_shape_tampers(S):
    report = []
    later = lambda seq, a, b: a if seq[a] > seq[b] else b
    flat = S.FlatProblem(racks())
    flat.solve(decode=False)

    def to_rack_63(res, seq, prob):
        k = [i for i in range(prob["K"]) if int(prob["key_nvalues"][i]) == 64]
        assert list(res["pod_node"]) == [63, 62] and len(k) == 1 and int(prob["en.mask"][63 * prob["K"] + k[0]]) == int(prob["en.mask"][64 * prob["K"] + k[0]]) == 1 << 63
        res["pod_node"][1] = 64      # another node of the rack rk_a's node is in: value id 63
    report.append((SHAPE_TAMPER_NAMES[0], _claim(S, flat, to_rack_63, B["ANTI_AFFINITY"], lambda res, seq: [later(seq, 0, 1)])))
    flat.close()
    flat = S.FlatProblem(many_groups())
    flat.solve(decode=False)

    def to_the_targets_zone(res, seq, prob):
        assert list(res["pod_node"]) == [0, 1] and seq[0] < seq[1]
        res["pod_node"][1] = 0
    report.append((SHAPE_TAMPER_NAMES[1], _claim(S, flat, to_the_targets_zone, B["ANTI_AFFINITY"], lambda res, seq: [1])))
    flat.close()
    return report
