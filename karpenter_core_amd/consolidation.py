"""Consolidation what-if fan-out across GPUs (BASELINE config #4).

Every deprovisioning what-if is an independent `simulateScheduling` (reference
pkg/controllers/deprovisioning/helpers.go:42-115): a pure function of (cluster snapshot, candidate set).
What-if i goes to rank i mod world; each rank solves its shard in ONE batched launch (one workgroup per
what-if, `scheduler.solve_batch`), and ONE all-gather of fixed-size result records returns everything the
reference's callers read from a simulation (consolidation.go:190-260):

    record = [whatif_id, n_new_nodes, n_unscheduled, first new node's InstanceTypeOptions as TW 64-bit words]

`allPodsScheduled` is n_unscheduled == 0; `len(newNodes)` gates replace-vs-delete; the option mask feeds
filterByPrice.  torch.distributed is plumbing only: backend "nccl" is RCCL over xGMI on the GPU box, "gloo"
in the CPU tests.  There is exactly one collective on the data path.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch
import torch.distributed as dist

from .model import Problem, SolveResult


def shard(n: int, rank: int, world: int) -> List[int]:
    """What-if indices owned by `rank` (round-robin: neighbouring prefixes have neighbouring cost)."""
    return list(range(rank, n, world))


def deal(weights: Sequence[int], world: int) -> List[List[int]]:
    """Which rank solves which what-if, by predicted work (e.g. the pods of its candidate nodes): longest first, each to the least loaded rank (ties: the lower rank) --
    the LPT rule, the same as include/ksolve.h ks_deal_lpt.  Round-robin (`shard`) leaves a step as long as its longest what-if plus whatever i mod N put beside it;
    this puts the longest what-if (nearly) alone.  Returns the what-if ids of every rank, ascending."""
    order = sorted(range(len(weights)), key=lambda i: (-int(weights[i]), i))
    load = [0] * world
    out: List[List[int]] = [[] for _ in range(world)]
    for i in order:
        r = min(range(world), key=lambda k: (load[k], k))
        out[r].append(i)
        load[r] += int(weights[i]) or 1
    return [sorted(x) for x in out]


def record_width(n_instance_types: int) -> int:
    return 3 + (n_instance_types + 63) // 64


def to_record(whatif_id: int, res: SolveResult, type_index: dict, width: int) -> torch.Tensor:
    rec = torch.zeros(width, dtype=torch.int64)
    rec[0], rec[1], rec[2] = whatif_id, len(res.new_nodes), len(res.unscheduled)
    if res.new_nodes:
        for name in res.new_nodes[0].instance_types:
            t = type_index[name]
            w = 3 + t // 64
            v = int(rec[w]) & 0xFFFFFFFFFFFFFFFF
            v |= 1 << (t % 64)
            rec[w] = v - (1 << 64) if v >= (1 << 63) else v
    return rec


def all_gather_records(records: torch.Tensor, per_rank: int) -> torch.Tensor:
    """The single exchange step of the sharded what-if path: this rank's [m, width] int64 result records (column 0 = what-if id, m <= per_rank)
    are padded to per_rank rows with id -1, all-gathered once, and returned as the full table ordered by what-if id (on `records`' device).
    Used by `solve_whatifs` and by `bench.py --gpus N`; a world of one returns the records sorted."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    width = records.shape[1]
    local = torch.full((per_rank, width), -1, dtype=torch.int64, device=records.device)
    local[: records.shape[0]] = records
    if world > 1:
        gathered = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(gathered, local)
        table = torch.cat(gathered, 0)
    else:
        table = local
    table = table[table[:, 0] >= 0]
    return table[torch.argsort(table[:, 0])]


def all_gather_grid_rows(rows, device: str = "cpu"):
    """The one exchange step of the sharded static grid (scheduler.sharded_grid): this rank's bit-rows (numpy uint64 [m, TW]; the ranks' shares differ by at
    most one row) all-gathered ONCE over the process group -- RCCL over xGMI with device="cuda", gloo on the CPU -- and handed back as one numpy array per rank, in rank order."""
    import numpy as np
    world = dist.get_world_size() if dist.is_initialized() else 1
    if world == 1:
        return [rows]
    tw = rows.shape[1]
    n = torch.tensor([rows.shape[0]], dtype=torch.int64, device=device)
    counts = [torch.empty_like(n) for _ in range(world)]
    dist.all_gather(counts, n)                                  # (the shares' sizes are a function of M * C and the world size; gathered so that a mismatch is loud, not silent)
    counts = [int(c.item()) for c in counts]
    per = max(counts)
    local = torch.zeros((per, tw), dtype=torch.int64, device=device)
    local[: rows.shape[0]] = torch.from_numpy(rows.view(np.int64)).to(device)
    gathered = [torch.empty_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    return [g[:c].cpu().numpy().view(np.uint64) for g, c in zip(gathered, counts)]


def solve_whatifs(problems: Sequence[Problem], solve_many: Callable[[List[Problem]], List[SolveResult]],
                  device: str = "cpu") -> torch.Tensor:
    """Solve all what-ifs across the process group; every rank returns the full [n, width] record table."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    n = len(problems)
    width = record_width(len(problems[0].instance_types)) if n else 3
    type_index = {it.name: i for i, it in enumerate(problems[0].instance_types)} if n else {}
    mine = shard(n, rank, world)
    results = solve_many([problems[i] for i in mine]) if mine else []
    per_rank = (n + world - 1) // world
    local = torch.full((len(mine), width), -1, dtype=torch.int64)
    for slot, (i, res) in enumerate(zip(mine, results)):
        local[slot] = to_record(i, res, type_index, width)
    return all_gather_records(local.to(device), per_rank).cpu()


def gpu_solve_many(problems: List[Problem], device: Optional[int] = None) -> List[SolveResult]:
    """One batched launch on this rank's GPU (no CPU path: raises without a gfx950 device).  `device` defaults to the calling
    rank's current HIP device (torch.cuda.current_device(), i.e. LOCAL_RANK after torch.cuda.set_device)."""
    from . import scheduler
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    flats = [scheduler.FlatProblem(p) for p in problems]
    try:
        for f in flats:
            f.upload(device)
        res, _, _ = scheduler.solve_batch(flats)
        return res
    finally:
        for f in flats:
            f.close()


# =====================================================================================================
# Consolidation decisions on top of the batched what-ifs.
#
# The reference runs ONE simulateScheduling per probe: ceil(log2 N) dependent Solves for multi-node
# consolidation's binary search (multinodeconsolidation.go:74-114), up to N sequential ones for single-node
# consolidation's first-success scan (singlenodeconsolidation.go:43-78).  Here every prefix / every singleton
# is solved in ONE ks_solve_batch launch, the price stage (filterByPrice over worstLaunchPrice,
# helpers.go:148-157,292-315) runs on the device over the results while they are still there, and the
# reference's control flow is replayed over the per-what-if commands.  Validation (validation.go: TTL wait,
# re-simulation) and events need the live cluster and stay in Go.
# =====================================================================================================
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

from .model import (InstanceType, LABEL_CAPACITY_TYPE, LABEL_INITIALIZED, LABEL_INSTANCE_TYPE, LABEL_ZONE, Provisioner,
                    RequirementOut, StateNode)

ACTION_DO_NOTHING, ACTION_DELETE, ACTION_REPLACE = "do-nothing", "delete", "replace"   # deprovisioning/types.go actions
CAPACITY_TYPE_SPOT, CAPACITY_TYPE_ON_DEMAND = "spot", "on-demand"


@dataclass
class Snapshot:
    """What candidateNodes / simulateScheduling read from the cluster (helpers.go:42-115, 165-230)."""
    instance_types: List[InstanceType]
    provisioner: Provisioner
    nodes: List[StateNode]
    bound: List[list]                      # pods bound to each node
    pending: list = field(default_factory=list)      # provisioner.GetPendingPods (helpers.go:76-79): they join the batch of every simulation
    deleting: tuple = ()                   # indices of nodes that are MarkedForDeletion (helpers.go:48-61): not state nodes, their pods join the batch


@dataclass
class CandidateNode:
    """deprovisioning CandidateNode (types.go): the node plus what pricing reads."""
    index: int
    name: str
    instance_type: str
    capacity_type: str
    zone: str


@dataclass
class Command:
    """deprovisioning Command as far as the decision goes: action, nodesToRemove, the replacement node's options."""
    action: str = ACTION_DO_NOTHING
    nodes_to_remove: List[str] = field(default_factory=list)
    replacement_types: List[str] = field(default_factory=list)                 # replacementNodes[0].InstanceTypeOptions
    replacement_requirements: Dict[str, tuple] = field(default_factory=dict)  # ... .Requirements (canonical tuples)
    error: Optional[str] = None     # computeConsolidation returned an error for this candidate set (consolidation.go:224-228)
    replacements: List[tuple] = field(default_factory=list)    # Expiration / Drift: EVERY replacement node as (InstanceTypeOptions, canonical Requirements), in new-node order

    def canonical(self):
        return (self.action, tuple(self.nodes_to_remove), tuple(self.replacement_types), tuple(sorted(self.replacement_requirements.items())))


class _NoProblem:
    def close(self):
        pass


def candidate(snapshot: Snapshot, i: int) -> CandidateNode:
    lab = snapshot.nodes[i].labels
    return CandidateNode(i, snapshot.nodes[i].name, lab[LABEL_INSTANCE_TYPE], lab[LABEL_CAPACITY_TYPE], lab[LABEL_ZONE])


def _offering_price(it: InstanceType, capacity_type: str, zone: str) -> Optional[float]:
    for o in it.offerings:                 # Offerings.Get, cloudprovider/types.go:117-124 (availability is not consulted)
        if o.capacity_type == capacity_type and o.zone == zone:
            return o.price
    return None


def get_node_prices(types: Dict[str, InstanceType], cands: Sequence[CandidateNode]) -> float:
    """getNodePrices, consolidation.go:277-287."""
    price = 0.0
    for c in cands:
        p = _offering_price(types[c.instance_type], c.capacity_type, c.zone)
        if p is None:
            raise ValueError(f"unable to determine offering for {c.instance_type}/{c.capacity_type}/{c.zone}")
        price += p
    return price


def _has(r: Optional[RequirementOut], value: str) -> bool:
    """Requirements.Get(key).Has(value): a missing key reads as Exists (requirements.go:114-120, requirement.go:171-176)."""
    if r is None:
        return True
    inside = value in r.values
    if (inside if r.complement else not inside):
        return False
    if r.greater_than is None and r.less_than is None:
        return True
    try:
        v = int(value)
    except ValueError:
        return False
    return not ((r.greater_than is not None and r.greater_than >= v) or (r.less_than is not None and r.less_than <= v))


def _req_tuple(r: RequirementOut) -> tuple:
    return (r.complement, tuple(sorted(r.values)), r.greater_than, r.less_than)


def compute_consolidations(snapshot: Snapshot, candidate_sets: Sequence[Sequence[int]]) -> Tuple[List[Command], list, list]:
    """computeConsolidation (consolidation.go:190-274) for every candidate set at once: one batched Solve, one batched
    price stage.  Returns (commands, flat problems, results); the caller closes the flat problems."""
    from . import scheduler, workloads
    types = {it.name: it for it in snapshot.instance_types}
    tindex = {it.name: i for i, it in enumerate(snapshot.instance_types)}
    # one snapshot, flattened natively per what-if on all host cores (scheduler.open_whatifs)
    # simulateScheduling's batch is pending pods + the candidates' pods + the pods of nodes that are already deleting (helpers.go:76-84), and
    # deleting nodes are no state nodes (:48-55).  Over the shared snapshot: the pending pods sit on a node of their own that no provisioner owns
    # (it is never an existing node) and that every candidate set removes first; the deleting nodes are removed last.
    PENDING = "~pending~"
    deleting = [int(j) for j in snapshot.deleting]
    nodes, bound = list(snapshot.nodes), list(snapshot.bound)
    pend_idx = None
    if snapshot.pending:
        pend_idx = len(nodes)
        nodes.append(StateNode(name=PENDING)); bound.append(list(snapshot.pending))
    snap, pod_node = workloads.snapshot_problem(snapshot.instance_types, snapshot.provisioner, nodes, bound)
    snap.cluster_pods = [cp for cp in snap.cluster_pods if cp.node_name != PENDING]      # pending pods are bound nowhere: countDomains does not see them
    cmds = [Command() for _ in candidate_sets]
    live = [i for i, cs in enumerate(candidate_sets) if not (set(cs) & set(deleting))]
    for i in range(len(candidate_sets)):
        if i not in set(live):
            cmds[i] = Command(error="candidate node is deleting")       # errCandidateNodeDeleting, helpers.go:62-67
    sets = [([pend_idx] if pend_idx is not None else []) + list(candidate_sets[i]) + deleting for i in live]
    flats_live = scheduler.open_whatifs(snap, pod_node, sets)
    results_live, _, _ = scheduler.solve_batch(flats_live) if flats_live else ([], 0, 0)
    flats = [_NoProblem()] * len(candidate_sets); results = [None] * len(candidate_sets)       # (a refused candidate set has nothing on the device)
    for i, f, r in zip(live, flats_live, results_live):
        flats[i], results[i] = f, r
    need, prices = [], []
    for i, (cs, res) in enumerate(zip(candidate_sets, results)):
        if res is None:
            continue
        cands = [candidate(snapshot, j) for j in cs]
        # simulateScheduling, helpers.go:102-111: the simulation must not lean on a node that is not ready yet -- Solve returns EVERY
        # in-state existing node (scheduler.go:132), so one uninitialised node that stays in the cluster fails the simulation
        removed = set(cs) | set(deleting)
        if any(n.owned and n.labels.get(LABEL_INITIALIZED) != "true" for j, n in enumerate(snapshot.nodes) if j not in removed and n.in_state):
            continue
        if res.unscheduled:                                     # "not all pods would schedule"
            continue
        if not res.new_nodes:                                   # everything fits on the remaining nodes
            cmds[i] = Command(ACTION_DELETE, [c.name for c in cands])
            continue
        if len(res.new_nodes) != 1:                             # "we're not going to turn a single node into multiple nodes"
            continue
        try:
            price = get_node_prices(types, cands)
        except ValueError as e:                                 # "getting offering price from candidate node": an error of THIS computation only
            cmds[i] = Command(error=str(e))
            continue
        need.append(i)
        prices.append(price)
    kept = scheduler.price_filter([flats[i] for i in need], [0] * len(need), prices)
    for i, keep in zip(need, kept):
        res = results[i]
        node = res.new_nodes[0]
        keep = set(keep)
        options = [n for n in node.instance_types if tindex[n] in keep]   # filterByPrice preserves the option order
        if not options:                                         # "can't replace with a cheaper node"
            continue
        cands = [candidate(snapshot, j) for j in candidate_sets[i]]
        ct = node.requirements.get(LABEL_CAPACITY_TYPE)
        if all(c.capacity_type == CAPACITY_TYPE_SPOT for c in cands) and _has(ct, CAPACITY_TYPE_SPOT):
            continue                                            # "can't replace a spot node with a spot node"
        reqs = {k: _req_tuple(r) for k, r in node.requirements.items()}
        if _has(ct, CAPACITY_TYPE_SPOT) and _has(ct, CAPACITY_TYPE_ON_DEMAND):
            # OD -> [OD, spot] was priced on the spot assumption: pin the launch to spot (Requirements.Add = intersection)
            reqs[LABEL_CAPACITY_TYPE] = (False, (CAPACITY_TYPE_SPOT,), None, None)
        cmds[i] = Command(ACTION_REPLACE, [c.name for c in cands], options, reqs)
    return cmds, flats, results


def simulate_candidates(snapshot: Snapshot, candidate_sets: Sequence[Sequence[int]]) -> List[Optional[SolveResult]]:
    """simulateScheduling (helpers.go:42-99) for every candidate set in ONE batched launch over the shared snapshot; None where the reference returns
    errCandidateNodeDeleting."""
    from . import scheduler, workloads
    PENDING = "~pending~"
    deleting = [int(j) for j in snapshot.deleting]
    nodes, bound = list(snapshot.nodes), list(snapshot.bound)
    pend_idx = None
    if snapshot.pending:
        pend_idx = len(nodes)
        nodes.append(StateNode(name=PENDING)); bound.append(list(snapshot.pending))
    snap, pod_node = workloads.snapshot_problem(snapshot.instance_types, snapshot.provisioner, nodes, bound)
    snap.cluster_pods = [cp for cp in snap.cluster_pods if cp.node_name != PENDING]
    live = [i for i, cs in enumerate(candidate_sets) if not (set(cs) & set(deleting))]
    sets = [([pend_idx] if pend_idx is not None else []) + list(candidate_sets[i]) + deleting for i in live]
    flats = scheduler.open_whatifs(snap, pod_node, sets) if sets else []
    got, _, _ = scheduler.solve_batch(flats) if flats else ([], 0, 0)
    for f in flats:
        f.close()
    out: List[Optional[SolveResult]] = [None] * len(candidate_sets)
    for i, r in zip(live, got):
        out[i] = r
    return out


def replacement_command(snapshot: Snapshot, candidates: Sequence[int], simulate: Optional[Callable] = None):
    """Drift.ComputeCommand / Expiration.ComputeCommand (drift.go:59-98, expiration.go:68-113) after their candidate filters and sort.  The reference
    simulates candidate after candidate and stops at the first whose simulation runs; here every candidate is simulated in ONE batch (`simulate`, default
    `simulate_candidates`) and the same first candidate decides: delete if its pods fit the rest of the cluster, otherwise replace it with EVERY node the
    simulation opened (no price stage, any number of nodes; pods left unscheduled are only logged there).
    -> (action, [node name], [(instance type options, canonical requirements)] per replacement node)"""
    results = (simulate or simulate_candidates)(snapshot, [[i] for i in candidates])
    for i, res in zip(candidates, results):
        if res is None:                                        # errCandidateNodeDeleting: "just retry" with the next candidate
            continue
        name = snapshot.nodes[i].name
        if not res.new_nodes:
            return (ACTION_DELETE, [name], [])
        return (ACTION_REPLACE, [name], [(list(n.instance_types), tuple(sorted((k, _req_tuple(r)) for k, r in n.requirements.items()))) for n in res.new_nodes])
    return (ACTION_DO_NOTHING, [], [])


def validate_command(snapshot: Snapshot, cmd: Command, candidates: Sequence[int], simulate: Optional[Callable] = None) -> bool:
    """Validation.ValidateCommand (validation.go:109-172) on the cluster as it is NOW (the TTL wait before it stays with the caller): the command's nodes
    that are still candidates are simulated again -- valid iff every pod schedules and the simulation needs no new node where none was expected, or exactly
    one whose instance type options contain the command's (instanceTypesAreSubset: the simulation applies no price filter, so it may list more)."""
    names = {snapshot.nodes[i].name: i for i in candidates}
    idx = [names[n] for n in cmd.nodes_to_remove if n in names]
    if not idx:
        return False
    (res,) = (simulate or simulate_candidates)(snapshot, [idx])
    if res is None:
        raise ValueError("candidate node is deleting")          # "simulating scheduling, %w"
    removed = set(idx) | set(int(j) for j in snapshot.deleting)
    if any(n.owned and n.labels.get(LABEL_INITIALIZED) != "true" for j, n in enumerate(snapshot.nodes) if j not in removed and n.in_state):
        return False                                             # helpers.go:102-111: allPodsScheduled = false
    if res.unscheduled:
        return False
    if not res.new_nodes:
        return not cmd.replacement_types
    if len(res.new_nodes) > 1 or not cmd.replacement_types:
        return False
    return set(cmd.replacement_types) <= set(res.new_nodes[0].instance_types)


def _filter_out_same_type(snapshot: Snapshot, flat, result, cmd: Command, cands: Sequence[CandidateNode]) -> List[str]:
    """filterOutSameType, multinodeconsolidation.go:132-165 (the second filterByPrice runs on the device as well)."""
    from . import scheduler
    types = {it.name: it for it in snapshot.instance_types}
    tindex = {it.name: i for i, it in enumerate(snapshot.instance_types)}
    existing, by_type = set(), {}
    for c in cands:
        existing.add(c.instance_type)
        p = _offering_price(types[c.instance_type], c.capacity_type, c.zone)
        if p is None:
            continue
        if p < by_type.get(c.instance_type, float("inf")) or c.instance_type not in by_type:
            by_type[c.instance_type] = min(p, by_type.get(c.instance_type, 1.7976931348623157e308))
    max_price = 1.7976931348623157e308
    for n in cmd.replacement_types:
        if n in existing and by_type.get(n, 0.0) < max_price:   # a Go map miss reads 0.0
            max_price = by_type.get(n, 0.0)
    # computeConsolidation may have narrowed the replacement's capacity-type to spot after pricing; the device still holds the
    # Solve's requirements, so the second pricing is told about the narrowing
    narrowed = cmd.replacement_requirements.get(LABEL_CAPACITY_TYPE) == (False, (CAPACITY_TYPE_SPOT,), None, None)   # idempotent if it already was
    keep = set(scheduler.price_filter([flat], [0], [max_price], [narrowed])[0])
    return [n for n in cmd.replacement_types if tindex[n] in keep]


def first_n_node_consolidation_option(snapshot: Snapshot, candidates: Sequence[int], max_nodes: int = 100) -> Command:
    """firstNNodeConsolidationOption, multinodeconsolidation.go:74-114: every prefix the binary search could probe is
    solved in one launch, then the search is replayed over the commands."""
    if len(candidates) < 2:
        return Command()
    lo, hi = 1, max_nodes
    if len(candidates) <= hi:
        hi = len(candidates) - 1
    prefixes = [list(candidates[0:mid + 1]) for mid in range(lo, hi + 1)]
    cmds, flats, results = compute_consolidations(snapshot, prefixes)
    try:
        last = Command()
        while lo <= hi:
            mid = (lo + hi) // 2
            k = mid - 1
            action = cmds[k]
            if action.error is not None:                        # firstNNodeConsolidationOption returns the error of the prefix it probes (:92-95)
                raise ValueError(action.error)
            if action.action == ACTION_REPLACE:
                cands = [candidate(snapshot, j) for j in prefixes[k]]
                opts = _filter_out_same_type(snapshot, flats[k], results[k], action, cands)
                action = Command(ACTION_REPLACE if opts else ACTION_DO_NOTHING, action.nodes_to_remove if opts else [], opts,
                                 action.replacement_requirements if opts else {})
            if action.action in (ACTION_REPLACE, ACTION_DELETE):
                last = action
                lo = mid + 1
            else:
                hi = mid - 1
        return last
    finally:
        for f in flats:
            f.close()


def single_node_consolidation_option(snapshot: Snapshot, candidates: Sequence[int]) -> Command:
    """SingleNodeConsolidation.ComputeCommand's scan, singlenodeconsolidation.go:54-78 (validation stays in Go): every
    singleton in one launch, first replace/delete in candidate order wins."""
    cmds, flats, _ = compute_consolidations(snapshot, [[c] for c in candidates])
    for f in flats:
        f.close()
    for cmd in cmds:
        if cmd.error is not None:                               # logged, next candidate (singlenodeconsolidation.go:57-60)
            continue
        if cmd.action in (ACTION_REPLACE, ACTION_DELETE):
            return cmd
    return Command()


# =====================================================================================================
# The same three decisions through the C ABI's command rows (include/kshost.h ksh_consolidation_commands, ksh_first_n_node_option, ksh_single_node_option): the
# what-ifs are derived, solved and DECIDED on the device (ks_consolidation_commands, csrc/ksolve.hip); no result is decoded on the host, the price stage makes no
# second trip.  Same Command objects as the functions above, which stay as they are.
# =====================================================================================================
_CMD_ERRORS = {4: "unable to determine offering for a candidate node", 10: "candidate node is deleting"}


def _command_snapshot(snapshot: Snapshot):
    """The snapshot as the C ABI takes it: (ParsedProblem, pod_node, nodes that leave every what-if -- the carrier of the pending pods, then the deleting nodes)."""
    from . import scheduler, workloads
    PENDING = "~pending~"
    nodes, bound = list(snapshot.nodes), list(snapshot.bound)
    leaving = []
    if snapshot.pending:
        leaving.append(len(nodes))
        nodes.append(StateNode(name=PENDING)); bound.append(list(snapshot.pending))
    leaving += [int(j) for j in snapshot.deleting]
    snap, pod_node = workloads.snapshot_problem(snapshot.instance_types, snapshot.provisioner, nodes, bound)
    snap.cluster_pods = [cp for cp in snap.cluster_pods if cp.node_name != PENDING]      # pending pods are bound nowhere: countDomains does not see them
    return scheduler.ParsedProblem(snap), pod_node, leaving


def _command_of_row(snapshot: Snapshot, parsed, row, words: int, cands: Sequence[int], second_stage: bool = False) -> Command:
    from . import scheduler as S
    d = S.decode_command_row(parsed, row, words)
    if d["action"] == S.KS_CMD_ERROR:
        return Command(error=_CMD_ERRORS.get(d["reason"], "error"))
    names = [snapshot.nodes[j].name for j in cands]
    if d["action"] == S.KS_CMD_DELETE:
        return Command(ACTION_DELETE, names)
    if d["action"] != S.KS_CMD_REPLACE:
        return Command()
    keep = set(d["options_same_type"] if second_stage else d["options"])
    options = [snapshot.instance_types[t].name for t in snapshot.provisioner.instance_types if t in keep]      # filterByPrice preserves the option order (lo.Filter)
    return Command(ACTION_REPLACE, names, options, d["requirements"])


def _words(snapshot: Snapshot) -> int:
    return (len(snapshot.instance_types) + 63) // 64


def _lists_flag(group_lists: bool) -> int:
    """`group_lists` of the `*_dev` calls that simulate what-ifs: kshost.h KSH_DERIVE_GROUP_LISTS -- the what-ifs are derived on the device for any number of topology
    groups (per-node lists) instead of falling back to the host above 1024.  The commands are the same either way."""
    from . import scheduler as S
    return S.KSH_DERIVE_GROUP_LISTS if group_lists else 0


def compute_consolidations_dev(snapshot: Snapshot, candidate_sets: Sequence[Sequence[int]], timings: Optional[dict] = None, group_lists: bool = False) -> List[Command]:
    """`compute_consolidations` through `ksh_consolidation_commands`: one call, one command per candidate set.  `timings` (a dict) receives the call's open / solve /
    command kernel / read-back milliseconds."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        rows, ms = S.consolidation_commands(parsed, pod_node, candidate_sets, _words(snapshot), deleting=leaving, flags=_lists_flag(group_lists))
        if timings is not None:
            timings.update(ms)
        return [_command_of_row(snapshot, parsed, rows[i], _words(snapshot), cs) for i, cs in enumerate(candidate_sets)]
    finally:
        parsed.close()


def first_n_node_consolidation_option_dev(snapshot: Snapshot, candidates: Sequence[int], max_nodes: int = 100, timings: Optional[dict] = None, group_lists: bool = False) -> Command:
    """`first_n_node_consolidation_option` through `ksh_first_n_node_option`: every prefix AND its filterOutSameType in one batch, the search replayed in the library."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        row, ms = S.first_n_node_option(parsed, pod_node, candidates, _words(snapshot), max_nodes=max_nodes, deleting=leaving, flags=_lists_flag(group_lists))
        if timings is not None:
            timings.update(ms)
        cmd = _command_of_row(snapshot, parsed, row, _words(snapshot), list(candidates[: int(row[S.KS_CMD_ID])]), second_stage=True)
        if cmd.error is not None:
            raise ValueError(cmd.error)
        return cmd
    finally:
        parsed.close()


def single_node_consolidation_option_dev(snapshot: Snapshot, candidates: Sequence[int], timings: Optional[dict] = None, group_lists: bool = False) -> Command:
    """`single_node_consolidation_option` through `ksh_single_node_option`."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        row, ms = S.single_node_option(parsed, pod_node, candidates, _words(snapshot), deleting=leaving, flags=_lists_flag(group_lists))
        if timings is not None:
            timings.update(ms)
        if (int(row[S.KS_CMD_DECISION]) & 0xFF) == S.KS_CMD_DO_NOTHING:
            return Command()
        return _command_of_row(snapshot, parsed, row, _words(snapshot), [candidates[int(row[S.KS_CMD_ID])]])
    finally:
        parsed.close()


@dataclass
class CandidateInfo:
    """What candidate selection reads beside the snapshot's objects (kshost.h `ksh_candidate_inputs`), per node and per bound pod of a `Snapshot`."""
    node_age_seconds: List[float]
    nominated: Sequence[int] = ()                       # node indices
    do_not_consolidate: Dict[int, str] = field(default_factory=dict)      # node index -> the annotation's value
    deletion_timestamp: Sequence[int] = ()              # node indices
    do_not_evict: Sequence[str] = ()                    # pod uids
    deletion_cost: Dict[str, float] = field(default_factory=dict)         # pod uid -> the parsed annotation
    priority: Dict[str, int] = field(default_factory=dict)                # pod uid -> Spec.Priority
    consolidation_enabled: bool = True
    ttl_seconds_until_expired: Optional[int] = None
    pdbs: Sequence = ()                                 # model.PodDisruptionBudget
    # expiration / drift / emptiness (kshost.h `ksh_deprovisioning_inputs`); the defaults leave every consolidation use as it is
    now_unix_nanos: int = 0                             # clock.Now()
    node_creation_unix_nanos: Sequence[int] = ()        # per node; missing entries read 0
    emptiness_unix_nanos: Dict[int, Optional[int]] = field(default_factory=dict)      # node index -> the parsed emptiness timestamp; None: it does not parse
    drifted: Sequence[int] = ()                         # node indices whose voluntary-disruption annotation says "drifted"
    drift_enabled: bool = False
    ttl_seconds_after_empty: Optional[int] = None


def _candidates_call(S, parsed, pod_node, snapshot: Snapshot, info: CandidateInfo, device: int = 0, wide_selectors: bool = False):
    """`ksh_consolidation_candidates` over a `Snapshot` opened by `_command_snapshot`: (the call's result over every node slot, the node flags it was given)."""
    pods = [p for b in snapshot.bound for p in b] + list(snapshot.pending)
    nn = len(snapshot.nodes) + (1 if snapshot.pending else 0)
    nf = [0] * nn
    for i in info.nominated:
        nf[i] |= S.KSH_CAND_NODE_NOMINATED
    for i, v in info.do_not_consolidate.items():
        nf[i] |= S.KSH_CAND_NODE_DO_NOT_CONSOLIDATE | (S.KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE if v == "true" else 0)
    for i in info.deletion_timestamp:
        nf[i] |= S.KSH_CAND_NODE_DELETION_TIMESTAMP
    dne = set(info.do_not_evict)
    pf = [(S.KSH_CAND_POD_DO_NOT_EVICT if p.uid in dne else 0) | (S.KSH_CAND_POD_HAS_DELETION_COST if p.uid in info.deletion_cost else 0) |
          (S.KSH_CAND_POD_HAS_PRIORITY if p.uid in info.priority else 0) for p in pods]
    age = list(info.node_age_seconds) + [0.0] * (nn - len(info.node_age_seconds))
    got = S.consolidation_candidates(parsed, pod_node, nf, age, pf, [float(info.deletion_cost.get(p.uid, 0.0)) for p in pods], [int(info.priority.get(p.uid, 0)) for p in pods],
                                     [info.consolidation_enabled], [info.ttl_seconds_until_expired], pdbs=info.pdbs, deleting=[int(j) for j in snapshot.deleting], device=device,
                                     wide_selectors=wide_selectors)
    return got, nf


def consolidation_candidates_dev(snapshot: Snapshot, info: CandidateInfo, device: int = 0, timings: Optional[dict] = None, wide_selectors: bool = False) -> dict:
    """candidateNodes + ShouldDeprovision + sortAndFilterCandidates through `ksh_consolidation_candidates`: {"order": the candidates' node indices by disruption
    cost -- what `first_n_node_consolidation_option_dev` / `single_node_consolidation_option_dev` take as they are --, "empty": the candidates without pods in the same
    order, "why" / "detail" / "cost" / "n_node_pods" per node (kshost.h lists the reason codes)}.  Pending pods and their carrier node are not candidates' business:
    only the snapshot's own nodes are reported.  `wide_selectors`: KSH_CAND_WIDE_SELECTORS -- PDB selectors of any number of keys, values and set sizes."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        got, _ = _candidates_call(S, parsed, pod_node, snapshot, info, device, wide_selectors)
        if timings is not None:
            timings.update(got["ms"])
        n = len(snapshot.nodes)
        return {"order": got["order"], "empty": got["empty"], "why": [int(x) for x in got["why"][:n]], "detail": [int(x) for x in got["detail"][:n]],
                "cost": [float(x) for x in got["cost"][:n]], "n_node_pods": [int(x) for x in got["n_node_pods"][:n]]}
    finally:
        parsed.close()


from .scheduler import KSH_METHOD_EXPIRATION as METHOD_EXPIRATION, KSH_METHOD_DRIFT as METHOD_DRIFT, KSH_METHOD_EMPTINESS as METHOD_EMPTINESS      # noqa: E402  (one definition)


def _deprovisioning_call(S, parsed, pod_node, snapshot: Snapshot, info: CandidateInfo, method: int, device: int = 0, wide_selectors: bool = False):
    """`ksh_deprovisioning_candidates` over a `Snapshot` opened by `_command_snapshot`."""
    pods = [p for b in snapshot.bound for p in b] + list(snapshot.pending)
    nn = len(snapshot.nodes) + (1 if snapshot.pending else 0)
    nf = [0] * nn
    for i in info.nominated:
        nf[i] |= S.KSH_CAND_NODE_NOMINATED
    for i in info.deletion_timestamp:
        nf[i] |= S.KSH_CAND_NODE_DELETION_TIMESTAMP
    for i in info.drifted:
        nf[i] |= S.KSH_CAND_NODE_DRIFTED
    for i, t in info.emptiness_unix_nanos.items():
        nf[i] |= S.KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP | (S.KSH_CAND_NODE_EMPTINESS_UNPARSABLE if t is None else 0)
    dne = set(info.do_not_evict)
    pf = [(S.KSH_CAND_POD_DO_NOT_EVICT if p.uid in dne else 0) | (S.KSH_CAND_POD_HAS_DELETION_COST if p.uid in info.deletion_cost else 0) |
          (S.KSH_CAND_POD_HAS_PRIORITY if p.uid in info.priority else 0) for p in pods]
    pad = lambda xs, fill: list(xs) + [fill] * (nn - len(xs))
    return S.deprovisioning_candidates(parsed, method, pod_node, info.now_unix_nanos, nf, pad(info.node_creation_unix_nanos, 0), pad(info.node_age_seconds, 0.0), pf,
                                       [float(info.deletion_cost.get(p.uid, 0.0)) for p in pods], [int(info.priority.get(p.uid, 0)) for p in pods], [info.ttl_seconds_until_expired],
                                       [info.ttl_seconds_after_empty], [info.emptiness_unix_nanos.get(i) or 0 for i in range(nn)], drift_enabled=info.drift_enabled, pdbs=info.pdbs,
                                       deleting=[int(j) for j in snapshot.deleting], device=device, wide_selectors=wide_selectors)


def deprovisioning_candidates_dev(snapshot: Snapshot, info: CandidateInfo, method: int, device: int = 0, timings: Optional[dict] = None, wide_selectors: bool = False) -> dict:
    """candidateNodes under Expiration / Drift / Emptiness.ShouldDeprovision (`method`: METHOD_*) through `ksh_deprovisioning_candidates`: `consolidation_candidates_dev`'s
    dict plus "n_in_result".  "order" is what Expiration / Drift.ComputeCommand walk (`replacement_command` takes it as it is); under emptiness it is the whole command."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        got = _deprovisioning_call(S, parsed, pod_node, snapshot, info, method, device, wide_selectors)
        if timings is not None:
            timings.update(got["ms"])
        n = len(snapshot.nodes)
        return {"order": got["order"], "empty": got["empty"], "why": [int(x) for x in got["why"][:n]], "detail": [int(x) for x in got["detail"][:n]],
                "cost": [float(x) for x in got["cost"][:n]], "n_node_pods": [int(x) for x in got["n_node_pods"][:n]], "n_in_result": got["n_in_result"]}
    finally:
        parsed.close()


def emptiness_command_dev(snapshot: Snapshot, info: CandidateInfo, device: int = 0) -> Command:
    """Emptiness: candidates on the device, then Emptiness.ComputeCommand (`ksh_emptiness_command`): every empty node past its ttl deleted in one command."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        got = _deprovisioning_call(S, parsed, pod_node, snapshot, info, METHOD_EMPTINESS, device)
        action, nodes = S.emptiness_command(got["order"], got["n_node_pods"])
        return Command(ACTION_DELETE, [snapshot.nodes[i].name for i in nodes]) if action == S.KS_CMD_DELETE else Command()
    finally:
        parsed.close()


def _replacement_command_dev(snapshot: Snapshot, info: CandidateInfo, method: int, device: int, timings: Optional[dict], group_lists: bool = False) -> Command:
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        got = _deprovisioning_call(S, parsed, pod_node, snapshot, info, method, device)
        if got["n_in_result"] == 0:
            return Command()
        words = _words(snapshot)
        head, nodes, _, pos, ms = S.replacement_option(parsed, pod_node, got["order"], got["why"], words, deleting=leaving, device=device, flags=_lists_flag(group_lists))
        if timings is not None:
            timings.update(ms)
        h = S.decode_replacement_head(head)
        if pos < 0 or h["action"] not in (S.KS_CMD_DELETE, S.KS_CMD_REPLACE):
            return Command()
        name = [snapshot.nodes[got["order"][pos]].name]
        if h["action"] == S.KS_CMD_DELETE:
            return Command(ACTION_DELETE, name)
        reps = []
        for row in nodes[h["node_off"]:h["node_off"] + h["n_nodes"]]:
            d = S.decode_replacement_node(parsed, row, words)
            keep = set(d["options"])
            reps.append(([snapshot.instance_types[t].name for t in snapshot.provisioner.instance_types if t in keep], tuple(sorted(d["requirements"].items()))))
        return Command(ACTION_REPLACE, name, list(reps[0][0]), dict(reps[0][1]), replacements=reps)
    finally:
        parsed.close()


def expiration_command_dev(snapshot: Snapshot, info: CandidateInfo, device: int = 0, timings: Optional[dict] = None, group_lists: bool = False) -> Command:
    """Expiration through the C ABI: `ksh_deprovisioning_candidates` (most expired first), then `ksh_replacement_option` -- ONE what-if simulated.  Command.replacements
    lists every replacement node.  Follows the reference where `replacement_command` does not: an uninitialised node that stays makes the command a plain delete."""
    return _replacement_command_dev(snapshot, info, METHOD_EXPIRATION, device, timings, group_lists)


def drift_command_dev(snapshot: Snapshot, info: CandidateInfo, device: int = 0, timings: Optional[dict] = None, group_lists: bool = False) -> Command:
    """Drift through the C ABI: one drifted node at a time, in slot order."""
    return _replacement_command_dev(snapshot, info, METHOD_DRIFT, device, timings, group_lists)


# =====================================================================================================
# Validation through the C ABI (include/kshost.h ksh_validate_commands, ksh_single_node_resume, ksh_validate_empty_nodes): `snapshot_now` is the cluster after
# consolidationTTL; node and instance-type NAMES are translated to slots and bits of that snapshot.  `validate_command` above stays as it is.
# =====================================================================================================
def _command_inputs_now(snapshot_now: Snapshot, commands: Sequence[Command]):
    slot = {n.name: i for i, n in enumerate(snapshot_now.nodes)}
    tindex = {it.name: i for i, it in enumerate(snapshot_now.instance_types)}
    for cmd in commands:
        for t in cmd.replacement_types:
            if t not in tindex:
                raise ValueError(f"replacement type {t} is not in the catalogue of the snapshot passed")
    node_sets = [[slot[n] for n in cmd.nodes_to_remove if n in slot] for cmd in commands]      # (a node that is not in the cluster any more cannot map)
    return node_sets, [bool(cmd.replacement_types) for cmd in commands], [[tindex[t] for t in cmd.replacement_types] for cmd in commands]


def validate_commands_dev(snapshot_now: Snapshot, commands: Sequence[Command], info: CandidateInfo, device: int = 0, timings: Optional[dict] = None,
                          group_lists: bool = False) -> List[Tuple[Optional[bool], int]]:
    """Validation.IsValid (after its wait) for every command in ONE call: candidates over `snapshot_now` (`ksh_consolidation_candidates`), then `ksh_validate_commands`.
    -> [(valid, why)] per command; valid is None where the reference returns an error (a node of the command that is still a candidate is being deleted); why: ksolve.h
    KS_VAL_WHY_*."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot_now)
    try:
        got, nf = _candidates_call(S, parsed, pod_node, snapshot_now, info, device)
        node_sets, expect, type_sets = _command_inputs_now(snapshot_now, commands)
        rows, ms = S.validate_commands(parsed, pod_node, node_sets, expect, type_sets, got["why"], nf, _words(snapshot_now), deleting=leaving, device=device, flags=_lists_flag(group_lists))
        if timings is not None:
            timings.update(ms)
        out = []
        for row in rows:
            d = S.decode_validation_row(row, _words(snapshot_now))
            out.append((d["valid"], d["why"]))
        return out
    finally:
        parsed.close()


def single_node_resume_dev(snapshot_now: Snapshot, candidates: Sequence[int], failed_before: bool, info: CandidateInfo, device: int = 0, timings: Optional[dict] = None,
                           group_lists: bool = False) -> Tuple[str, Command]:
    """The rest of SingleNodeConsolidation.ComputeCommand's loop after a validation has failed, through `ksh_single_node_resume`: `candidates` are the node indices (of
    `snapshot_now`) that follow the failed one.  -> ("found", the valid command) | ("retry", Command()) | ("do-nothing", Command())."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot_now)
    try:
        got, nf = _candidates_call(S, parsed, pod_node, snapshot_now, info, device)
        state, row, _, ms = S.single_node_resume(parsed, pod_node, candidates, failed_before, got["why"], nf, _words(snapshot_now), deleting=leaving, device=device, flags=_lists_flag(group_lists))
        if timings is not None:
            timings.update(ms)
        if state != 1:
            return ("retry" if state == 2 else "do-nothing"), Command()
        return "found", _command_of_row(snapshot_now, parsed, row, _words(snapshot_now), [candidates[int(row[S.KS_CMD_ID])]])
    finally:
        parsed.close()


def validate_empty_nodes(snapshot_now: Snapshot, node_names: Sequence[str], info: CandidateInfo, device: int = 0) -> bool:
    """EmptyNodeConsolidation's check after its wait (emptynodeconsolidation.go:77-87) through `ksh_validate_empty_nodes`: True = retry.  A command none of whose nodes
    is still a candidate is NOT a retry: the reference returns it as it is."""
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot_now)
    try:
        got, nf = _candidates_call(S, parsed, pod_node, snapshot_now, info, device)
        slot = {n.name: i for i, n in enumerate(snapshot_now.nodes)}
        return S.validate_empty_nodes([slot[n] for n in node_names if n in slot], got["why"], got["n_node_pods"], nf)
    finally:
        parsed.close()


# =====================================================================================================
# Provisioning over the same snapshot (include/kshost.h ksh_provision): Provisioner.Reconcile's Solve (provisioning/provisioner.go:117-150) is
# simulateScheduling with no candidate -- `snapshot.pending` plus the pods of `snapshot.deleting` against the nodes that stay.
# =====================================================================================================
@dataclass
class Provisioning:
    """What `NewScheduler(...).Solve` returns (scheduler.go:96), plus what the launch needs: `nodes` are scheduler.Node with Pods in commit order, `existing`
    scheduler.ExistingNode for the state nodes that took pods, `unscheduled` [(pod, packed reason word)] in queue order, `stages` {pod uid: relaxation stage > 0} to
    apply back to pod.Spec, `picks` per new node (instance type name, zone, capacity type, price) or None -- the in-memory provider's launch pick --, `route` how the
    what-if was made ("derived" / "flattened" / "nothing")."""
    nodes: list = field(default_factory=list)
    existing: list = field(default_factory=list)
    unscheduled: list = field(default_factory=list)
    stages: dict = field(default_factory=dict)
    picks: list = field(default_factory=list)
    route: str = "nothing"


def provision_dev(snapshot: Snapshot, info: Optional["CandidateInfo"] = None, device: int = 0, timings: Optional[dict] = None, group_lists: bool = False, volumes: bool = False,
                  active_resources: bool = False) -> Provisioning:
    """Provisioner.Reconcile's scheduling pass through `ksh_provision`: one call, one what-if, the rows decoded into the shapes Solve returns.  `info` is accepted so
    that the call reads like the other `*_dev` passes over a snapshot; provisioning reads nothing of it (no candidate is chosen)."""
    import ctypes
    from . import scheduler as S
    parsed, pod_node, leaving = _command_snapshot(snapshot)
    try:
        words = _words(snapshot)
        got = S.provision(parsed, pod_node, leaving, words, device=device, flags=_lists_flag(group_lists), volumes=volumes, active_resources=active_resources)
        if timings is not None:
            timings.update(got["ms"])
        out = Provisioning(route=got["route"])
        if got["route"] == "nothing":
            return out
        pods = [p for b in snapshot.bound for p in b] + list(snapshot.pending)      # the snapshot's pod order: _command_snapshot binds the pending pods to the carrier, the last node
        head = got["head"]
        lists = S.placement_lists([S.decode_placement_row(r, head["n_existing"]) for r in got["rows"]])
        kh = S.libs()[1]
        kh.ksh_snapshot_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        kh.ksh_snapshot_name.restype = ctypes.c_char_p
        for j in range(head["n_new"]):
            d = S.decode_replacement_node(parsed, got["machines"][j], words)
            keep = set(d["options"])
            reqs = {k: RequirementOut(k, v[0], tuple(v[1]), v[2], v[3]) for k, v in d["requirements"].items()}
            out.nodes.append(S.Node(snapshot.provisioner.name, [pods[i] for i in lists["new"].get(j, [])], [snapshot.instance_types[t] for t in snapshot.provisioner.instance_types if t in keep],
                                    reqs, d["requests"]))
            pk = got["picks"][j]
            out.picks.append(None if pk is None else (snapshot.instance_types[pk[0]].name, kh.ksh_snapshot_name(parsed._p, 5, pk[1], 0).decode(), kh.ksh_snapshot_name(parsed._p, 6, pk[2], 0).decode(), pk[3]))
        out.existing = [S.ExistingNode(snapshot.nodes[slot], [pods[i] for i in idxs]) for slot, idxs in sorted(lists["existing"].items())]
        out.unscheduled = [(pods[i], lists["reasons"][i]) for i in lists["unscheduled"]]
        out.stages = {pods[i].uid: st for i, st in lists["stage"].items() if st > 0}
        return out
    finally:
        parsed.close()
