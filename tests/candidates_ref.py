"""A literal Python restatement of the first step of a consolidation pass in the reference -- which nodes are candidates, and in what order -- for
tests/test_consolidation_candidates.py.  Nothing here is shared with the product: plain objects in, plain lists out.  Python floats are IEEE doubles, so every
cost below has the bits the Go code computes.

  GetPodEvictionCost / disruptionCost / calculateLifetimeRemaining / clamp     deprovisioning/helpers.go:124-165, 275-287, 317-325
  candidateNodes                                                               helpers.go:171-249
  consolidation.ShouldDeprovision / sortAndFilterCandidates                    consolidation.go:83-121
  canBeTerminated / PodsPreventEviction                                        helpers.go:339-366
  PDBLimits.CanEvictPods                                                       pdblimits.go:55-70
  labels.Selector.Matches of metav1.LabelSelectorAsSelector                    k8s.io/apimachinery: In / NotIn / Exists / DoesNotExist; nil selects nothing

Two things the reference leaves open are fixed the way the project fixes them everywhere: cluster.ForEachNode walks a map and sort.Slice is unstable, so the
canonical execution walks the nodes in ascending slot order and sorts stably; GetNodePods' list is the node's bound pods in ascending slot order."""
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

PROVISIONER_NAME = "karpenter.sh/provisioner-name"
INSTANCE_TYPE = "node.kubernetes.io/instance-type"
CAPACITY_TYPE = "karpenter.sh/capacity-type"
ZONE = "topology.kubernetes.io/zone"
INITIALIZED = "karpenter.sh/initialized"


@dataclass
class RPod:
    slot: int
    namespace: str
    labels: Dict[str, str]
    do_not_evict: bool = False
    deletion_cost: Optional[float] = None      # the parsed annotation; None: absent
    priority: Optional[int] = None             # Spec.Priority; None: nil


@dataclass
class RNode:
    labels: Dict[str, str]
    pods: List[RPod] = field(default_factory=list)      # GetNodePods, ascending slot
    left: bool = False                          # the slot's node is gone (not walked by ForEachNode)
    marked_for_deletion: bool = False
    nominated: bool = False
    do_not_consolidate: Optional[str] = None    # the annotation's value; None: absent
    deletion_timestamp: bool = False
    age_seconds: float = 0.0


@dataclass
class RProvisioner:
    name: str
    instance_types: List[str]
    consolidation_enabled: bool = True
    ttl_seconds_until_expired: Optional[int] = None


@dataclass
class RPdb:
    namespace: str
    selector: object            # None (nil) or an object with match_labels {k: v} and match_expressions [(key, op, values)]
    disruptions_allowed: int


def clamp(lo, val, hi):
    if val < lo:
        return lo
    if val > hi:
        return hi
    return val


def get_pod_eviction_cost(p: RPod) -> float:
    cost = 1.0
    if p.deletion_cost is not None:
        cost += p.deletion_cost / math.pow(2, 27.0)
    if p.priority is not None:
        cost += float(p.priority) / math.pow(2, 25)
    return clamp(-10.0, cost, 10.0)


def disruption_cost(pods) -> float:
    cost = 0.0
    for p in pods:
        cost += get_pod_eviction_cost(p)
    return cost


def calculate_lifetime_remaining(ttl_seconds_until_expired, age_seconds) -> float:
    remaining = 1.0
    if ttl_seconds_until_expired is not None:
        total = float(ttl_seconds_until_expired)
        left = total - age_seconds
        remaining = clamp(0.0, left / total, 1.0)
    return remaining


def selector_matches(sel, labels: Dict[str, str]) -> bool:
    if sel is None:                      # LabelSelectorAsSelector(nil) = labels.Nothing()
        return False
    for k, v in sel.match_labels.items():
        if labels.get(k) != v or k not in labels:
            return False
    for e in sel.match_expressions:
        key, op, values = e.key, e.op, e.values
        if op == "In":
            if key not in labels or labels[key] not in values:
                return False
        elif op == "NotIn":
            if key in labels and labels[key] in values:
                return False
        elif op == "Exists":
            if key not in labels:
                return False
        elif op == "DoesNotExist":
            if key in labels:
                return False
        else:
            raise ValueError(op)
    return True


def can_evict_pods(pdbs: List[RPdb], pods):
    for pod in pods:
        for i, pdb in enumerate(pdbs):
            if pdb.namespace == pod.namespace:
                if selector_matches(pdb.selector, pod.labels):
                    if pdb.disruptions_allowed == 0:
                        return i, False
    return None, True


def pods_prevent_eviction(pods):
    for p in pods:
        if p.do_not_evict:
            return p.slot, True
    return None, False


def candidates(nodes: List[RNode], provisioners: List[RProvisioner], pdbs: List[RPdb]) -> dict:
    provs = {p.name: p for p in provisioners}
    n = len(nodes)
    why, detail, cost = [0] * n, [-1] * n, [0.0] * n
    listed = []
    for i, nd in enumerate(nodes):
        if nd.left:
            why[i] = 13
            continue
        provisioner = provs.get(nd.labels[PROVISIONER_NAME]) if PROVISIONER_NAME in nd.labels else None
        if nd.marked_for_deletion:
            why[i] = 1
            continue
        if provisioner is None:
            why[i] = 2
            continue
        if nd.labels.get(INSTANCE_TYPE, "") not in provisioner.instance_types:
            why[i] = 3
            continue
        if CAPACITY_TYPE not in nd.labels:
            why[i] = 4
            continue
        if ZONE not in nd.labels:
            why[i] = 5
            continue
        if nd.labels.get(INITIALIZED) != "true":
            why[i] = 6
            continue
        if nd.nominated:
            why[i] = 7
            continue
        # ShouldDeprovision
        if nd.do_not_consolidate is not None:
            if not (nd.do_not_consolidate != "true"):
                why[i] = 8
                continue
        elif not provisioner.consolidation_enabled:
            why[i] = 9
            continue
        c = disruption_cost(nd.pods)
        c *= calculate_lifetime_remaining(provisioner.ttl_seconds_until_expired, nd.age_seconds)
        cost[i] = c
        listed.append(i)
    kept = []
    for i in listed:                       # sortAndFilterCandidates: canBeTerminated
        nd = nodes[i]
        if nd.deletion_timestamp:
            why[i] = 10
            continue
        pdb, ok = can_evict_pods(pdbs, nd.pods)
        if not ok:
            why[i], detail[i] = 11, pdb
            continue
        slot, prevents = pods_prevent_eviction(nd.pods)
        if prevents:
            why[i], detail[i] = 12, slot
            continue
        kept.append(i)
    # a stable sort on `cost <` (Python's sort is stable; the key compares as float64 does: -0.0 == 0.0)
    import functools
    order = sorted(kept, key=functools.cmp_to_key(lambda a, b: -1 if cost[a] < cost[b] else (1 if cost[b] < cost[a] else 0)))
    return {"order": order, "empty": [i for i in order if len(nodes[i].pods) == 0], "why": why, "detail": detail, "cost": cost,
            "n_node_pods": [len(nd.pods) for nd in nodes]}
