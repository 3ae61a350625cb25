"""Problems for one STEP of ks_pack_rr's RUN rounds, shared by tests/test_rr_run_steps.py (lane-fibre emulator) and tests/test_rr_run_steps_gpu.py.

A step has every worker wave publish its accepting keys of ONE count bucket -- all of them, each by the lane that holds it, when the wave has at most eight; its eight
smallest, one wave minimum each, when it has more or an existing node leads -- and, after the merge, has the lanes that hold the winners commit side by side.  The
shapes below are the smallest at which each piece of that can go wrong.  Node n lives in worker wave n % 7, lane (n % 448) / 7, register slot n / 448.

The generators are tests/long_runs_cases.py's (openers that each need a machine of their own, plain replicas behind them)."""
from karpenter_core_amd import fake
from karpenter_core_amd.model import (Container, DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_ZONE, LabelSelector, Offering, Pod, PodAffinityTerm, TopologySpreadConstraint)

import long_runs_cases as LC

WAVES, LANE_NODES = 7, 448      # worker waves; nodes per register slot (RR_NODE_AT)


def _anti_opener(uid, cpu, mem):
    return Pod(uid=uid, labels={"role": "opener"}, containers=[Container(requests={"cpu": cpu, "memory": mem})],
               anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"role": "opener"}))])


PAIRS = 11


def one_lane_two_winners(replicas=80):
    """Nodes 0..10 and 448..458 -- slots 0 and 1 of the SAME lanes -- are the only ones that accept: the first 11 openers (most cpu: first in the queue) leave their
    machines' memory free, the 437 openers B behind them fill theirs, the last 11 (nodes 448..) are small; the replicas need memory and sort last (least cpu).  The head
    window places its few replicas on the first nodes; from then on a step's winners are node n AND node n + 448 for one n after the other: one lane commits both.
    (With nodes 0 and 448 alone the stretch never reaches RUN rounds: the window holds node 0 and not node 448, places a replica on it, meets one it cannot place --
    a round takes that one -- and so on in turn.)"""
    pods = [_anti_opener(f"a1-open-{i:02d}", "8000m", "512Mi") for i in range(PAIRS)]
    pods += [_anti_opener(f"b-open-{i:05d}", "4000m", "250Gi") for i in range(LANE_NODES - PAIRS)]
    pods += [_anti_opener(f"c2-open-{i:02d}", "2000m", "512Mi") for i in range(PAIRS)]
    pods += [Pod(uid=f"r-mem-{i:05d}", labels={"app": "web"}, containers=[Container(requests={"cpu": "100m", "memory": "8Gi"})]) for i in range(replicas)]
    return LC._problem([LC._box(160)], pods)


def pairs_take_the_replicas(res):
    """(the oracle's placements of one_lane_two_winners) the replicas went to nodes 0..10 and 448..458 and to no other, and every one of those took some: a count
    bucket of the run holds node n and node n + 448 together"""
    took = {i for i, n in enumerate(res.new_nodes) if len(n.pods) > 1}
    return took == set(range(PAIRS)) | set(range(LANE_NODES, LANE_NODES + PAIRS)) and len(res.new_nodes) == LANE_NODES + PAIRS


def more_than_eight_in_one_wave(openers=141, replicas=60):
    """Worker wave 0 holds MORE than eight accepting nodes of the bucket and the other waves hold one each, late in the order: every seventh machine (nodes 0, 7, ..
    133) and the last seven (134 .. 140) have memory left, the others are full (the openers' cpu falls from one to the next: the queue keeps them in this order
    whatever their memory).  Wave 0 publishes its eight smallest and FLAGS the eighth; without the flag the step would go on with node 134 where node 112 is next."""
    pods = [_anti_opener(f"a-open-{i:03d}", f"{10000 - 10 * i}m", "512Mi" if i % WAVES == 0 or i >= openers - WAVES else "250Gi") for i in range(openers)]
    pods += [Pod(uid=f"r-mem-{i:05d}", labels={"app": "web"}, containers=[Container(requests={"cpu": "100m", "memory": "8Gi"})]) for i in range(replicas)]
    return LC._problem([LC._box(160)], pods)


def only_these_take_replicas(nodes):
    return lambda res: {i for i, n in enumerate(res.new_nodes) if len(n.pods) > 1} == set(nodes)


def spread_in_two_groups(openers=20, lead=12, size=40):
    """Replicas of one base class under a hostname spread at maxSkew 1, in two groups of equal items (one selector each): rr_run_group cuts the run where the items
    change, a node takes one pod of a group and refuses the next (the retry reads the counter the commit wrote), and every commit counts a record."""
    pods = [LC._opener(i) for i in range(openers)] + [LC._replica(i) for i in range(lead)]
    i = lead
    for grp in ("ga", "gb"):
        for _ in range(size):
            pods.append(LC._replica(i, labels={"grp": grp}, spread=[TopologySpreadConstraint(1, LABEL_HOSTNAME, DO_NOT_SCHEDULE, LabelSelector({"grp": grp}))]))
            i += 1
    return LC._problem([LC._box(160)], pods)


def zone_selector_on_open_machines(openers=20, replicas=80):
    """Replicas with a zone selector land on machines that unconstrained pods opened: the first commit on a node narrows its requirements (another requirement
    class: `rchg`), the later ones find the class they bring."""
    pods = [LC._opener(i) for i in range(openers)] + [LC._replica(i, node_selector={LABEL_ZONE: "test-zone-2"}) for i in range(replicas)]
    return LC._problem([LC._box(160)], pods)


def narrowing_changes_the_capacity(openers=7, replicas=60):
    """Two instance types, the larger one offered in test-zone-1 only: a machine opened by an unconstrained pod may still be either; a replica that selects
    test-zone-2 leaves the smaller one, with another capacity -- the exact filter has to look (the run stops at that pod: kind 3), then the run goes on."""
    def it(name, cpu, mem, zones):
        res = {"cpu": cpu, "memory": mem, "pods": "160"}
        return fake.new_instance_type(name, res, [Offering("on-demand", z, fake.price_from_resources(res)) for z in zones])
    its = [it("box", "64", "256Gi", ["test-zone-1", "test-zone-2"]), it("huge", "128", "512Gi", ["test-zone-1"])]
    pods = [LC._opener(i) for i in range(openers)] + [LC._replica(i, node_selector={LABEL_ZONE: "test-zone-2"}) for i in range(replicas)]
    return LC._problem(its, pods)


# name -> (maker, what the oracle's placements must show: a function of the oracle's result, or None)
CASES = {
    "fast_path_several_waves": (lambda: LC.stretch(60, openers=20), None),
    "bucket_of_56": (lambda: LC.stretch(200, openers=56), None),             # eight accepting keys in every wave: all published side by side
    "bucket_of_57": (lambda: LC.stretch(200, openers=57), None),             # ... one wave with nine: that one extracts one by one and flags its eighth
    "bucket_of_63": (lambda: LC.stretch(200, openers=63), None),             # ... nine in every wave
    "more_than_eight_in_one_wave": (more_than_eight_in_one_wave, only_these_take_replicas(list(range(0, 134, WAVES)) + list(range(134, 141)))),
    "two_slots_in_one_lane": (lambda: LC.stretch(300, openers=LANE_NODES + 12), None),      # nodes 448.. stand in slot 1 of the lanes that hold nodes 0.. in slot 0
    "one_lane_two_winners": (one_lane_two_winners, pairs_take_the_replicas),
    "existing_nodes_lead": (lambda: LC.existing_nodes(replicas=120, existing=3, free=12), None),
    "spread_in_two_groups": (spread_in_two_groups, None),
    "zone_selector_on_open_machines": (zone_selector_on_open_machines, None),
    "narrowing_changes_the_capacity": (narrowing_changes_the_capacity, None),
}
