"""A literal Python restatement of the three deprovisioning methods the reference's controller tries before consolidation (deprovisioning/controller.go:142-162), for
tests/test_deprovisioning_candidates.py.  CPU only, nothing shared with the product; every time is a Python integer of unix nanoseconds, so no sum rounds or wraps.

  candidateNodes                                   deprovisioning/helpers.go:171-249 (shared with tests/candidates_ref.py: steps 1-7, the cost, canBeTerminated)
  Expiration.ShouldDeprovision / SortCandidates    expiration.go:56-66, getExpirationTime :120-127
  Drift.ShouldDeprovision                          drift.go:50-56
  Emptiness.ShouldDeprovision                      emptiness.go:52-70
  Expiration / Drift.ComputeCommand                expiration.go:68-113, drift.go:59-98: the first candidate canBeTerminated lets through that is not deleting is simulated
  Emptiness.ComputeCommand                         emptiness.go:73-82
  simulateScheduling's readiness rule              helpers.go:102-113: an owned, in-state node that stays and is not initialised -> `nil, false, nil`, so len(newNodes) == 0

The open points are fixed as everywhere in the project: ForEachNode walks the slots in ascending order, sort.Slice is executed stably."""
from dataclasses import dataclass, field
from typing import List, Optional

import candidates_ref as R

EXPIRATION, DRIFT, EMPTINESS = 1, 2, 3
NOT_EXPIRED, NOT_DRIFTED, NOT_EMPTY = 14, 15, 16
SECOND = 10 ** 9
DRIFTED = "drifted"
UNPARSABLE = "unparsable"


@dataclass
class DNode(R.RNode):
    creation_ns: int = 0
    emptiness: object = None                     # None: no annotation; UNPARSABLE: time.Parse fails; else unix nanoseconds
    voluntary_disruption: Optional[str] = None   # the annotation's value


@dataclass
class DProvisioner(R.RProvisioner):
    ttl_seconds_after_empty: Optional[int] = None


def get_expiration_time(node: DNode, provisioner: DProvisioner) -> Optional[int]:
    """None stands for time.Date(5000, ...): later than any `now`, and equal to itself in the sort."""
    if provisioner is None or provisioner.ttl_seconds_until_expired is None:
        return None
    return node.creation_ns + provisioner.ttl_seconds_until_expired * SECOND


def should_deprovision(method, node: DNode, provisioner: DProvisioner, now: int, drift_enabled: bool):
    """-> (ok, detail of the clause that said no)"""
    if method == EXPIRATION:
        t = get_expiration_time(node, provisioner)
        if t is None:
            return False, 0
        return (True, -1) if now > t else (False, 1)
    if method == DRIFT:
        if not drift_enabled:
            return False, 0
        return (True, -1) if node.voluntary_disruption == DRIFTED else (False, 1)
    if provisioner is None or provisioner.ttl_seconds_after_empty is None:
        return False, 0
    if len(node.pods) != 0:
        return False, 1
    if node.emptiness is None:
        return False, 2
    if node.emptiness == UNPARSABLE:
        return True, -1
    return (True, -1) if now > node.emptiness + provisioner.ttl_seconds_after_empty * SECOND else (False, 3)


def candidates(method: int, nodes: List[DNode], provisioners: List[DProvisioner], pdbs: List[R.RPdb], now: int, drift_enabled: bool = False) -> dict:
    provs = {p.name: p for p in provisioners}
    n = len(nodes)
    why, detail, cost = [0] * n, [-1] * n, [0.0] * n
    listed = []
    for i, nd in enumerate(nodes):
        if nd.left:
            why[i] = 13
            continue
        provisioner = provs.get(nd.labels[R.PROVISIONER_NAME]) if R.PROVISIONER_NAME in nd.labels else None
        if nd.marked_for_deletion:
            why[i] = 1
        elif provisioner is None:
            why[i] = 2
        elif nd.labels.get(R.INSTANCE_TYPE, "") not in provisioner.instance_types:
            why[i] = 3
        elif R.CAPACITY_TYPE not in nd.labels:
            why[i] = 4
        elif R.ZONE not in nd.labels:
            why[i] = 5
        elif nd.labels.get(R.INITIALIZED) != "true":
            why[i] = 6
        elif nd.nominated:
            why[i] = 7
        if why[i]:
            continue
        ok, clause = should_deprovision(method, nd, provisioner, now, drift_enabled)
        if not ok:
            why[i], detail[i] = {EXPIRATION: NOT_EXPIRED, DRIFT: NOT_DRIFTED, EMPTINESS: NOT_EMPTY}[method], clause
            continue
        cost[i] = R.disruption_cost(nd.pods) * R.calculate_lifetime_remaining(provisioner.ttl_seconds_until_expired, nd.age_seconds)
        listed.append(i)
    n_in_result = len(listed)
    if method == EXPIRATION:      # SortCandidates, stably; `Before` over equal times is false both ways
        far = max([get_expiration_time(nodes[i], provs[nodes[i].labels[R.PROVISIONER_NAME]]) for i in listed] + [0]) + 1
        listed.sort(key=lambda i: (lambda t: far if t is None else t)(get_expiration_time(nodes[i], provs[nodes[i].labels[R.PROVISIONER_NAME]])))
    order = []
    for i in listed:
        nd = nodes[i]
        if method != EMPTINESS:      # ComputeCommand's canBeTerminated test; Emptiness.ComputeCommand has none
            if nd.deletion_timestamp:
                why[i] = 10
                continue
            pdb, ok = R.can_evict_pods(pdbs, nd.pods)
            if not ok:
                why[i], detail[i] = 11, pdb
                continue
            slot, prevents = R.pods_prevent_eviction(nd.pods)
            if prevents:
                why[i], detail[i] = 12, slot
                continue
        order.append(i)
    return {"order": order, "empty": [i for i in order if len(nodes[i].pods) == 0], "why": why, "detail": detail, "cost": cost, "n_node_pods": [len(nd.pods) for nd in nodes],
            "n_in_result": n_in_result}


def emptiness_command(order, n_node_pods):
    """Emptiness.ComputeCommand over candidateNodes' result: (action, nodes to remove)."""
    empty = [i for i in order if n_node_pods[i] == 0]
    return ("delete", empty) if empty else ("do-nothing", [])


def replacement_command(snapshot, order, simulate):
    """Expiration / Drift.ComputeCommand after the sort and canBeTerminated (`order`): `simulate(snapshot, i)` is simulateScheduling for candidate i alone and returns the
    new nodes as a list, or raises ValueError for errCandidateNodeDeleting.  With the readiness rule of helpers.go:102-113 the new nodes READ are none.
    -> (action, [node name], new nodes, position of the deciding candidate in `order` or -1)"""
    deleting = set(int(j) for j in getattr(snapshot, "deleting", ()))
    for pos, i in enumerate(order):
        try:
            new_nodes = simulate(snapshot, i)
        except ValueError:
            continue
        for j, n in enumerate(snapshot.nodes):
            if j != i and j not in deleting and n.in_state and n.owned and n.labels.get(R.INITIALIZED) != "true":
                new_nodes = []      # `return nil, false, nil`
                break
        name = snapshot.nodes[i].name
        if len(new_nodes) == 0:
            return ("delete", [name], [], pos)
        return ("replace", [name], list(new_nodes), pos)
    return ("do-nothing", [], [], -1)
