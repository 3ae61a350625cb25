"""What tests/test_audit.py (on the lane-fibre emulator) and tests/test_audit_gpu.py (on the device) share: the hand-made problem of the tamper matrix, the matrix
itself -- one minimal edit of a genuine result per audit bit, with the flags the edit must raise known by construction --, and the comparison of the device audit
with the reference audit (tests/audit_ref.py, through tests/audit_harness.py).  Every function takes the scheduler module `S` it is to go through (the HIP libraries' or the emulator's)."""
import copy

import numpy as np

import audit_harness as H
import audit_ref as A
from karpenter_core_amd import fake
from karpenter_core_amd.model import (LABEL_ARCH, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_OS, LABEL_PROVISIONER, LABEL_ZONE, NO_SCHEDULE, Container,
                                      HostPort, Offering, Pod, Problem, StateNode, Taint, Toleration, Volume)
from karpenter_core_amd.workloads import EBS_DRIVER

Z1, Z2, Z3 = "test-zone-1", "test-zone-2", "test-zone-3"
D = H.PASSES["audit"]      # the pass, and its comparison with the reference (tests/audit_harness.py)
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix's problem
def _pod(uid, cpu="100m", mem="64Mi", **kw):
    return Pod(uid=uid, containers=[Container(requests={"cpu": cpu, "memory": mem}, ports=kw.pop("ports", []))], **kw)


def _node(name, zone, cpu, taints=(), volume_limit=None):
    labels = {LABEL_PROVISIONER: "open", LABEL_INSTANCE_TYPE: "fake-it-5", LABEL_ZONE: zone, LABEL_CAPACITY_TYPE: "on-demand", LABEL_ARCH: "amd64", LABEL_OS: "linux",
              LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
    return StateNode(name=name, labels=labels, taints=list(taints), available={"cpu": cpu, "memory": "8Gi", "pods": "50"}, capacity={"cpu": "6", "memory": "12Gi", "pods": "60"},
                     volume_limits={EBS_DRIVER: volume_limit} if volume_limit is not None else {})


PODS = ["plain", "zonal", "named", "port_a", "port_b", "vol_a", "vol_b", "big", "limited_a", "limited_b", "huge"]


def tamper_problem() -> Problem:
    """Four existing nodes -- roomy (zone 1, one volume slot), tainted (zone 2), full (zone 1), second (zone 2) --, an open provisioner without limits and a tainted
    one with limits, seven types (the last offers nothing in zone 3).  Where the reference puts the pods (scheduler.go:96-219, first fit over the existing nodes
    in order): plain, zonal (zone 1), named (hostname In [roomy]), port_a and vol_a on roomy; port_b (the same host port) and vol_b (one volume too many for roomy)
    on second; big (zone 3, 2.5 cores) on a new node of the open provisioner; limited_a / limited_b (they name the limited provisioner and tolerate its taint) on a new
    node of that one; huge (64 cores) nowhere."""
    its = fake.instance_types(6)
    its.append(fake.new_instance_type("no-zone-3", {"cpu": "8", "memory": "16Gi", "pods": "80"}, [Offering("on-demand", Z1, 1.0), Offering("on-demand", Z2, 1.0)]))
    provs = [fake.provisioner("open", len(its), weight=10), fake.provisioner("limited", len(its), weight=1, taints=[Taint("dedicated", "limited", NO_SCHEDULE)], limits={"cpu": "100"})]
    nodes = [_node("roomy", Z1, "5", volume_limit=1), _node("tainted", Z2, "5", taints=[Taint("maintenance", "true", NO_SCHEDULE)]), _node("full", Z1, "50m"), _node("second", Z2, "5", volume_limit=4)]
    tol = [Toleration(key="dedicated", operator="Equal", value="limited", effect=NO_SCHEDULE)]
    pods = [_pod("plain"), _pod("zonal", node_selector={LABEL_ZONE: Z1}), _pod("named", cpu="1m", mem="1Mi", node_selector={LABEL_HOSTNAME: "roomy"}),
            _pod("port_a", ports=[HostPort(port=8080)]), _pod("port_b", ports=[HostPort(port=8080)]),
            _pod("vol_a", volumes=[Volume(EBS_DRIVER, "default/a")]), _pod("vol_b", volumes=[Volume(EBS_DRIVER, "default/b")]),
            _pod("big", cpu="2500m", mem="1Gi", node_selector={LABEL_ZONE: Z3}),
            _pod("limited_a", node_selector={LABEL_PROVISIONER: "limited"}, tolerations=tol), _pod("limited_b", node_selector={LABEL_PROVISIONER: "limited"}, tolerations=tol),
            _pod("huge", cpu="64")]
    assert [p.uid for p in pods] == PODS
    return Problem(instance_types=its, provisioners=provs, pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


ROOMY, TAINTED, FULL, SECOND = 0, 1, 2, 3


def check_genuine(res: dict) -> dict:
    """The genuine result is the one `tamper_problem` describes; returns where things are: pod name -> index, and the two new nodes."""
    pod = {n: i for i, n in enumerate(PODS)}
    E = 4
    assert res["n_existing"] == E and res["n_new"] == 2, (res["n_existing"], res["n_new"])
    where = {n: int(res["pod_node"][i]) for n, i in pod.items()}
    assert [where[n] for n in ("plain", "zonal", "named", "port_a", "vol_a")] == [ROOMY] * 5, where
    assert where["port_b"] == SECOND and where["vol_b"] == SECOND and where["huge"] == -1, where
    assert where["big"] >= E and where["limited_a"] >= E and where["limited_a"] == where["limited_b"] and where["big"] != where["limited_a"], where
    assert list(res["unscheduled"]) == [pod["huge"]]
    return {"pod": pod, "open": where["big"] - E, "limited": where["limited_a"] - E, "E": E}


def _move(res, prob, p, to, charge=False):
    """Pod p to node `to`.  charge: a new node's Requests take the pod's in -- the move then breaks nothing about the node's arithmetic."""
    res["pod_node"][p] = to
    if charge:
        c, R, j = int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + int(res["pod_stage"][p])]), prob["R"], to - prob["E"]
        res["node_requests"][j] += prob["cls_requests"][c * R:(c + 1) * R]
        res["node_requests_present"][j] |= prob["cls_requests_present"][c]


def tampers(res: dict, prob: dict):
    """[(name, edited copy of `res`, {pod index: pod bits}, {node index: node bits})]: one minimal edit per bit, the flags it must raise -- exactly those, on exactly
    those indices -- known from how `tamper_problem` was made."""
    g = check_genuine(res)
    pod, E, jo, jl, T = g["pod"], g["E"], g["open"], g["limited"], prob["T"]
    out = []

    def case(name, pods=None, nodes=None):
        r = copy.deepcopy({k: v for k, v in res.items() if k != "key_value"})
        out.append((name, r, pods or {}, nodes or {}))
        return r
    r = case("a pod moved to a full existing node", nodes={FULL: A.NODE["RESOURCES"]})
    _move(r, prob, pod["plain"], FULL)
    r = case("a pod moved to a node it does not tolerate", pods={pod["plain"]: A.POD["TAINTS"]})
    _move(r, prob, pod["plain"], TAINTED)
    r = case("a pod moved to a node in another zone than its selector", pods={pod["zonal"]: A.POD["REQUIREMENTS"]})
    _move(r, prob, pod["zonal"], SECOND)
    r = case("a hostname-In pod moved to a new node", pods={pod["named"]: A.POD["HOSTNAME"]})
    _move(r, prob, pod["named"], E + jo, charge=True)      # (1 milli-core, 1 Mi and one pod more: every option of the node still fits them)
    r = case("two port-conflicting pods on one node", pods={pod["port_a"]: A.POD["PORTS"], pod["port_b"]: A.POD["PORTS"]})
    _move(r, prob, pod["port_b"], ROOMY)
    r = case("a volume limit exceeded", nodes={ROOMY: A.NODE["VOLUMES"]})
    _move(r, prob, pod["vol_b"], ROOMY)
    r = case("node_requests off by one milli-unit", nodes={E + jo: A.NODE["REQUESTS"]})
    r["node_requests"][jo, 0] += 1
    assert not (int(res["node_types"][jo, 0]) >> 0) & 1 and not (int(res["node_types"][jo, 0]) >> (T - 1)) & 1      # genuine: neither the 1-core type nor the one without zone 3
    r = case("an option bit set for a type that is too small", nodes={E + jo: A.NODE["OPTIONS_EXTRA"]})
    r["node_types"][jo, 0] |= np.uint64(1)
    r = case("an option bit set for a type with no offering in the node's zone", nodes={E + jo: A.NODE["OPTIONS_EXTRA"]})
    r["node_types"][jo, 0] |= np.uint64(1 << (T - 1))
    for which, j, bits in (("an unlimited", jo, A.NODE["OPTIONS_MISSING"]), ("a limited", jl, 0)):
        have = int(res["node_types"][j, 0])
        assert bin(have).count("1") >= 2
        r = case("a valid option bit cleared, on %s template" % which, nodes={E + j: bits} if bits else {})
        r["node_types"][j, 0] = np.uint64(have & (have - 1))
    r = case("a pod dropped from unscheduled", pods={pod["huge"]: A.POD["UNSCHEDULED_LIST"]})
    r["unscheduled"] = r["unscheduled"][:0]
    r = case("a placed pod added to unscheduled", pods={pod["plain"]: A.POD["UNSCHEDULED_LIST"]})
    r["unscheduled"] = np.append(r["unscheduled"], np.int32(pod["plain"]))
    r = case("pod_stage past the pod's stages", pods={pod["plain"]: A.POD["RANGE"]})
    r["pod_stage"][pod["plain"]] = int(prob["pod_stage_off"][pod["plain"] + 1]) - int(prob["pod_stage_off"][pod["plain"]])
    r = case("a new node emptied", nodes={E + jo: A.NODE["EMPTY"]})
    r["pod_node"][pod["big"]] = -1
    r["unscheduled"] = np.append(r["unscheduled"], np.int32(pod["big"]))
    return out


def run_tamper_matrix(S):
    """Solve `tamper_problem`, audit the genuine result (clean) and every edit through the claimed form; returns [(name, ok or what differs)]."""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    assert_clean(S, flat)
    res, prob = flat.result_arrays(), A.problem_arrays(S, flat)
    report = []
    for name, claimed, pods, nodes in tampers(res, prob):
        want_p, want_n = np.zeros(prob["P"], dtype=np.uint32), np.zeros(prob["E"] + int(claimed["n_new"]), dtype=np.uint32)
        for i, b in pods.items():
            want_p[i] = b
        for i, b in nodes.items():
            want_n[i] = b
        try:
            dev, pf, nf = compare(S, flat, claimed)
            ok = np.array_equal(dev["pod_flags"], want_p) and np.array_equal(dev["node_flags"], want_n)
            report.append((name, True if ok else "pods %s nodes %s" % ({int(i): int(dev["pod_flags"][i]) for i in np.nonzero(dev["pod_flags"])[0]}, {int(i): int(dev["node_flags"][i]) for i in np.nonzero(dev["node_flags"])[0]})))
        except AssertionError as e:
            report.append((name, "device and reference audits differ: %s" % (e,)))
    flat.close()
    return report


TAMPER_NAMES = ["a pod moved to a full existing node", "a pod moved to a node it does not tolerate", "a pod moved to a node in another zone than its selector",
                "a hostname-In pod moved to a new node", "two port-conflicting pods on one node", "a volume limit exceeded", "node_requests off by one milli-unit",
                "an option bit set for a type that is too small", "an option bit set for a type with no offering in the node's zone",
                "a valid option bit cleared, on an unlimited template", "a valid option bit cleared, on a limited template", "a pod dropped from unscheduled",
                "a placed pod added to unscheduled", "pod_stage past the pod's stages", "a new node emptied"]
