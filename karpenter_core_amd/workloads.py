"""Seeded synthetic Solve() problems: the five BASELINE.json configs and the
reference benchmark's pod mix (scheduling_benchmark_test.go:185-288), restated.

Every generator returns a `model.Problem`; all randomness comes from numpy's legacy RandomState so a
seed pins the problem bit-for-bit on both the build container and the GPU box.
"""
from __future__ import annotations

from typing import List

import dataclasses

import numpy as np

from . import fake
from .model import (ClusterPod, Container, Expr, HostPort, LabelSelector, Pod, PodAffinityTerm, PreferredTerm, Problem, StateNode,
                    Taint, Toleration, TopologySpreadConstraint, DO_NOT_SCHEDULE, LABEL_ARCH, LABEL_CAPACITY_TYPE,
                    LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_OS, LABEL_PROVISIONER, LABEL_ZONE, NO_SCHEDULE, parse_quantity_milli)

CPU_CHOICES = [100, 250, 500, 1000, 1500]                 # scheduling_benchmark_test.go:285
MEM_CHOICES = [100, 256, 512, 1024, 2048, 4096]           # :280
LABEL_VALUES = ["a", "b", "c", "d", "e", "f", "g"]        # :275
ZONES = ["test-zone-1", "test-zone-2", "test-zone-3"]


def _container(rs) -> Container:
    return Container(requests={"cpu": f"{CPU_CHOICES[rs.randint(len(CPU_CHOICES))]}m",
                               "memory": f"{MEM_CHOICES[rs.randint(len(MEM_CHOICES))]}Mi"})


def _lab(rs) -> str:
    return LABEL_VALUES[rs.randint(len(LABEL_VALUES))]


def generic_pod(rs, uid) -> Pod:                           # makeGenericPods :235-250
    return Pod(uid=uid, labels={"my-label": _lab(rs)}, containers=[_container(rs)])


def spread_pod(rs, uid, key) -> Pod:                       # makeTopologySpreadPods :210-233
    return Pod(uid=uid, labels={"my-label": _lab(rs)}, containers=[_container(rs)],
               spread=[TopologySpreadConstraint(1, key, DO_NOT_SCHEDULE, LabelSelector({"my-label": _lab(rs)}))])


def affinity_pod(rs, uid, key) -> Pod:                     # makePodAffinityPods :199-208
    return Pod(uid=uid, labels={"my-affininity": _lab(rs)}, containers=[_container(rs)],
               affinity_required=[PodAffinityTerm(key, LabelSelector({"my-affininity": _lab(rs)}))])


def anti_affinity_pod(rs, uid, key, self_selecting=True) -> Pod:
    v = _lab(rs)
    sel = v if self_selecting else _lab(rs)
    return Pod(uid=uid, labels={"my-affininity": v}, containers=[_container(rs)],
               anti_required=[PodAffinityTerm(key, LabelSelector({"my-affininity": sel}))])


def diverse_pods(rs, count: int, uid_prefix="pod") -> List[Pod]:
    """makeDiversePods (:185-197): 1/7 generic, 1/7 zonal spread, 1/7 hostname spread, 1/7 hostname
    affinity, 1/7 zonal affinity, remainder generic.  UIDs are unique (the reference leaves them
    empty, which makes its queue order sort-implementation dependent -- SURVEY App. C.2)."""
    pods: List[Pod] = []
    n = count // 7
    k = [0]

    def uid():
        k[0] += 1
        return f"{uid_prefix}-{k[0]:07d}"
    pods += [generic_pod(rs, uid()) for _ in range(n)]
    pods += [spread_pod(rs, uid(), LABEL_ZONE) for _ in range(n)]
    pods += [spread_pod(rs, uid(), LABEL_HOSTNAME) for _ in range(n)]
    pods += [affinity_pod(rs, uid(), LABEL_HOSTNAME) for _ in range(n)]
    pods += [affinity_pod(rs, uid(), LABEL_ZONE) for _ in range(n)]
    pods += [generic_pod(rs, uid()) for _ in range(count - len(pods))]
    return pods


def reference_benchmark(pod_count: int, instance_count: int = 400, seed: int = 42) -> Problem:
    """benchmarkScheduler (:113-133): 1 provisioner, fake.InstanceTypes(n), makeDiversePods; run the
    oracle with inert_topology=True to mirror the reference's `&scheduling.Topology{}` (:123)."""
    rs = np.random.RandomState(seed)
    its = fake.instance_types(instance_count)
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its), limits={}, discovery_label=True)],
                   pods=diverse_pods(rs, pod_count), extra_well_known=fake.EXTRA_WELL_KNOWN)


# ---- config #1: 1k pods, 50 instance types, no affinity/topology ----
def config1(pods: int = 1000, types: int = 50, seed: int = 42) -> Problem:
    rs = np.random.RandomState(seed)
    its = fake.instance_types(types)
    ps = [Pod(uid=f"pod-{i:07d}", containers=[_container(rs)]) for i in range(pods)]
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=ps,
                   extra_well_known=fake.EXTRA_WELL_KNOWN)


TAINT_KEYS = [f"taint-{i}" for i in range(8)]


def _taint_catalogue(sizes, zone_sets, ct_sets):
    return fake.assorted_ladder(sizes, ["amd64", "arm64"], ["linux", "windows"], zone_sets, ct_sets)


# ---- config #2: 10k pods, 500 instance types, taints + nodeSelector ----
def config2(pods: int = 10_000, sizes: int = 25, seed: int = 43) -> Problem:
    rs = np.random.RandomState(seed)
    zone_sets = [[ZONES[0]], [ZONES[1]], [ZONES[2]], ZONES[:2], ZONES]
    its = _taint_catalogue(sizes, zone_sets, [["spot", "on-demand"]])        # sizes*2*2*5 types (500 at 25)
    n = len(its)
    # four tainted provisioners (weights 40..10) and one untainted catch-all; 4 of the 8 taint keys are used
    used = [int(x) for x in rs.choice(8, size=4, replace=False)]
    provs = []
    for i, tk in enumerate(used):
        taints = [Taint(TAINT_KEYS[tk], "true", NO_SCHEDULE)]
        if i == 0:
            taints.append(Taint(TAINT_KEYS[used[1]], "true", NO_SCHEDULE))
        provs.append(fake.provisioner(f"tainted-{i}", n, weight=40 - 10 * i, taints=taints))
    provs.append(fake.provisioner("default", n, weight=0))
    ps = []
    for i in range(pods):
        tol = [Toleration(key=TAINT_KEYS[k], operator="Exists", effect=NO_SCHEDULE) for k in range(8) if rs.rand() < 0.5]
        sel = {}
        if rs.rand() < 0.5:
            sel[LABEL_ARCH] = ["amd64", "arm64"][rs.randint(2)]
        if rs.rand() < 0.3:
            sel[LABEL_ZONE] = ZONES[rs.randint(3)]
        if rs.rand() < 0.2:
            sel[LABEL_CAPACITY_TYPE] = ["spot", "on-demand"][rs.randint(2)]
        ps.append(Pod(uid=f"pod-{i:07d}", labels={"my-label": _lab(rs)}, node_selector=sel, tolerations=tol,
                      containers=[_container(rs)]))
    return Problem(instance_types=its, provisioners=provs, pods=ps, extra_well_known=fake.EXTRA_WELL_KNOWN)


# ---- config #3: 100k pods, 2k instance types, topology spread + pod anti-affinity ----
def config3(pods: int = 100_000, sizes: int = 50, seed: int = 44) -> Problem:
    rs = np.random.RandomState(seed)
    zone_sets = [[ZONES[0]], [ZONES[1]], [ZONES[2]], ZONES[:2], ZONES]
    its = _taint_catalogue(sizes, zone_sets, [["spot", "on-demand"], ["on-demand"]])   # sizes*2*2*5*2 (2000 at 50)
    n = pods // 7
    ps: List[Pod] = []
    k = [0]

    def uid():
        k[0] += 1
        return f"pod-{k[0]:07d}"
    ps += [generic_pod(rs, uid()) for _ in range(n)]
    ps += [spread_pod(rs, uid(), LABEL_ZONE) for _ in range(n)]
    ps += [spread_pod(rs, uid(), LABEL_HOSTNAME) for _ in range(n)]
    ps += [anti_affinity_pod(rs, uid(), LABEL_HOSTNAME, True) for _ in range(n)]
    ps += [generic_pod(rs, uid()) for _ in range(pods - len(ps))]
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=ps,
                   extra_well_known=fake.EXTRA_WELL_KNOWN)


def hostname_herd(pods: int = 600, labels: int = 3, seed: int = 3) -> Problem:
    """Small pods that crowd the hostname-keyed groups: a third carry self-selecting hostname anti-affinity on one of `labels` values (a node takes one pod per value: the
    machines multiply, and once every node has its pod of a value the next pod of that value is taken by NOBODY), a third a hostname spread with maxSkew 1 on the
    same labels, the rest nothing.  What round 6's census of zero counters (ks_pack_rr: RRLds::hz) is about: counters leave 0 in the head window, in run steps, in
    normal rounds and when a machine opens with its first pod."""
    rs = np.random.RandomState(seed)
    its = fake.instance_types(8)
    ps: List[Pod] = []
    for i in range(pods):
        uid = f"pod-{i:07d}"
        c = Container(requests={"cpu": f"{[50, 100, 200][rs.randint(3)]}m", "memory": f"{[32, 64][rs.randint(2)]}Mi"})
        v = LABEL_VALUES[rs.randint(labels)]
        k = rs.randint(3)
        if k == 0:
            ps.append(Pod(uid=uid, labels={"my-affininity": v}, containers=[c], anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"my-affininity": v}))]))
        elif k == 1:
            ps.append(Pod(uid=uid, labels={"my-label": v}, containers=[c], spread=[TopologySpreadConstraint(1, LABEL_HOSTNAME, DO_NOT_SCHEDULE, LabelSelector({"my-label": v}))]))
        else:
            ps.append(Pod(uid=uid, labels={"my-label": v}, containers=[c]))
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=ps, extra_well_known=fake.EXTRA_WELL_KNOWN)


# ---- config #5: 1M pods, 5k instance types, full constraint set ----
def config5(pods: int = 1_000_000, sizes: int = 50, seed: int = 46) -> Problem:
    rs = np.random.RandomState(seed)
    zone_sets = [[ZONES[0]], [ZONES[1]], [ZONES[2]], ZONES[:2], ZONES]
    its = fake.assorted_ladder(sizes, ["amd64", "arm64"], ["linux", "windows"], zone_sets,
                               [["spot", "on-demand"], ["on-demand"], ["spot"], ["on-demand", "spot"], ["on-demand"]][: max(1, 5000 // (sizes * 20))])
    n = len(its)
    provs = [fake.provisioner("high", n, weight=10, limits={"cpu": str(max(1000, pods // 8))},
                              taints=[Taint(TAINT_KEYS[0], "true", NO_SCHEDULE)]),
             fake.provisioner("default", n, weight=0)]
    ps: List[Pod] = []
    for i in range(pods):
        kind = i % 10
        uid = f"pod-{i:07d}"
        tol = [Toleration(key=TAINT_KEYS[0], operator="Exists")] if rs.rand() < 0.3 else []
        c = _container(rs)
        if kind == 0:
            p = spread_pod(rs, uid, LABEL_ZONE)
        elif kind == 1:
            p = spread_pod(rs, uid, LABEL_HOSTNAME)
        elif kind == 2:
            p = spread_pod(rs, uid, LABEL_CAPACITY_TYPE)
        elif kind == 3:
            p = anti_affinity_pod(rs, uid, LABEL_HOSTNAME, True)
        elif kind == 4:
            p = affinity_pod(rs, uid, LABEL_ZONE)
        elif kind == 5:
            p = Pod(uid=uid, labels={"my-label": _lab(rs)}, containers=[c],
                    required_affinity=[[Expr(fake.LABEL_INTEGER, "Gt", [str(2 * (1 + rs.randint(8)))])]])
        else:
            p = generic_pod(rs, uid)
        p.tolerations = tol
        if rs.rand() < 0.01:
            p.containers[0].ports = [HostPort(port=8000 + int(rs.randint(4)))]
        if kind >= 6 and rs.rand() < 0.3:
            p.node_selector = {LABEL_ARCH: ["amd64", "arm64"][rs.randint(2)]}
        ps.append(p)
    return Problem(instance_types=its, provisioners=provs, pods=ps, extra_well_known=fake.EXTRA_WELL_KNOWN)


# ---- config #4: consolidation what-ifs over one cluster snapshot ----
def cluster_snapshot(existing: int = 2048, sizes: int = 50, seed: int = 45, spare_pod_slots: int = -1):
    """E existing (owned, initialised) nodes running 8-40 pods each at 30-70 % utilisation; returns
    (instance_types, provisioner, nodes, per-node bound pods as `Pod` objects).
    spare_pod_slots >= 0: a cluster that is full by pod COUNT (max-pods): only that many nodes, picked at random, keep 1-3 free pod slots, every
    other node has none -- the pods of a removed node then mostly need a NEW node (consolidation's "replace" outcome, consolidation.go:230-274)."""
    rs = np.random.RandomState(seed)
    zone_sets = [[ZONES[0]], [ZONES[1]], [ZONES[2]], ZONES[:2], ZONES]
    its = _taint_catalogue(sizes, zone_sets, [["spot", "on-demand"], ["on-demand"]])
    prov = fake.provisioner("default", len(its))
    nodes, bound = [], []
    uid = 0
    for e in range(existing):
        ti = int(rs.randint(len(its)))
        it = its[ti]
        cpu_m = int(it.capacity["cpu"]) * 1000 - 100
        mem_mi = int(it.capacity["memory"][:-2]) * 1024 - 10
        zone = it.offerings[rs.randint(len(it.offerings))]
        arch = [r for r in it.requirements if r.key == LABEL_ARCH][0].values[0]
        os_ = [r for r in it.requirements if r.key == LABEL_OS][0].values[0]
        target = rs.uniform(0.3, 0.7)
        npods = int(rs.randint(8, 41))
        pods_here, used_cpu, used_mem = [], 0, 0
        for _ in range(npods):
            p = generic_pod(rs, f"bound-{uid:07d}")
            uid += 1
            c = int(p.containers[0].requests["cpu"][:-1])
            m = int(p.containers[0].requests["memory"][:-2])
            if used_cpu + c > target * cpu_m or used_mem + m > target * mem_mi:
                break
            used_cpu += c
            used_mem += m
            pods_here.append(p)
        name = f"node-{e:05d}"
        labels = {LABEL_PROVISIONER: "default", LABEL_INSTANCE_TYPE: it.name, LABEL_ZONE: zone.zone,
                  LABEL_CAPACITY_TYPE: zone.capacity_type, LABEL_ARCH: arch, LABEL_OS: os_, LABEL_HOSTNAME: name,
                  "karpenter.sh/initialized": "true"}
        alloc_pods = int(it.capacity["pods"])
        nodes.append(StateNode(name=name, labels=labels,
                               available={"cpu": f"{cpu_m - used_cpu}m", "memory": f"{mem_mi - used_mem}Mi",
                                          "pods": str(alloc_pods - len(pods_here))},
                               capacity=dict(it.capacity)))
        bound.append(pods_here)
    if spare_pod_slots >= 0:
        rs2 = np.random.RandomState(seed + 1000)
        keep = set(int(x) for x in rs2.choice(existing, size=min(spare_pod_slots, existing), replace=False))
        for e, n in enumerate(nodes):
            n.available = dict(n.available, pods=str(int(rs2.randint(1, 4))) if e in keep else "0")
    return its, prov, nodes, bound


EBS_DRIVER, EFS_DRIVER, FSX_DRIVER = "ebs.csi.aws.com", "efs.csi.aws.com", "fsx.csi.aws.com"


def volume_snapshot(existing: int = 2048, sizes: int = 50, seed: int = 45, spare_pod_slots: int = -1, unowned: bool = True):
    """`cluster_snapshot` decorated like an EKS cluster with CSI drivers (state/cluster.go:292-304 VolumeLimits, volumeusage.go:102-143):
      - every owned node has a CSINode limit for the EBS driver (25 / 27 / 39; about one in six 2-4, so that limits bind), about a third one for EFS too;
        the FSx driver is mounted but no node limits it;
      - StatefulSet-like pods with 1-2 private EBS claims, RWX claims (EFS or EBS) mounted by pods on several nodes, a claim shared by two pods of one node,
        a few pods whose volume lookup failed (`volume_error`), and a few nodes already over one of their limits;
      - `unowned`: one more node, no provisioner owns it (index `existing`: no config #4 candidate set names it), whose pods mount claims only they mount and
        one of the RWX claims.
    A node's volume usage (`StateNode.volumes`) lists the claims of its bound pods, one entry per pod that mounts it (state/node.go:161-182 adds and removes
    per pod).  Returns (instance_types, provisioner, nodes, per-node bound pods) like `cluster_snapshot`."""
    from .model import Volume
    its, prov, nodes, bound = cluster_snapshot(existing, sizes, seed, spare_pod_slots)
    decorate_volumes(nodes, bound, np.random.RandomState(seed + 7000))
    if unowned and nodes:
        name = "unowned-0"
        pods = []
        for i, p in enumerate(bound[0][:4]):
            q = dataclasses.replace(p, uid=f"unowned-pod-{i}", volume_error=False,
                                    volumes=[Volume(EBS_DRIVER, f"default/orphan-{i}")] + ([Volume(EFS_DRIVER, "default/rwx-0000")] if i == 0 else []))
            pods.append(q)
        nodes.append(StateNode(name=name, labels={LABEL_ZONE: nodes[0].labels[LABEL_ZONE], LABEL_HOSTNAME: name}, volume_limits={EBS_DRIVER: 25},
                               volumes=[v for p in pods for v in p.volumes]))
        bound.append(pods)
    return its, prov, nodes, bound


def decorate_volumes(nodes, bound, rs):
    """`volume_snapshot`'s limits and claims on the owned nodes `nodes` and their pods `bound` (in place, drawn from the RandomState `rs`)."""
    from .model import Volume
    n_rwx = max(2, len(nodes) // 16)
    sts = 0
    for e, (n, pods) in enumerate(zip(nodes, bound)):
        n.volume_limits = {EBS_DRIVER: int(rs.choice([25, 27, 39])) if rs.rand() >= 0.16 else int(rs.randint(2, 5))}
        if rs.rand() < 0.33:
            n.volume_limits[EFS_DRIVER] = int(rs.randint(3, 9))
        for p in pods:
            r = rs.rand()
            if r < 0.25:
                p.volumes = [Volume(EBS_DRIVER, f"default/data-sts-{sts:06d}-{k}") for k in range(1 + int(rs.rand() < 0.4))]
                sts += 1
            elif r < 0.32:
                p.volumes = [Volume(EFS_DRIVER if rs.rand() < 0.6 else EBS_DRIVER, f"default/rwx-{int(rs.randint(n_rwx)):04d}")]
            elif r < 0.35:
                p.volumes = [Volume(FSX_DRIVER, f"default/scratch-{int(rs.randint(n_rwx)):04d}")]
            elif r < 0.36:
                p.volume_error = True
        if len(pods) >= 2 and rs.rand() < 0.2:
            pair = Volume(EBS_DRIVER, f"default/pair-{e:05d}")
            pods[0].volumes = pods[0].volumes + [pair]
            pods[1].volumes = pods[1].volumes + [pair]
        n.volumes = [v for p in pods for v in p.volumes]
        if rs.rand() < 0.03:
            ebs = len({v.pvc_id for v in n.volumes if v.driver == EBS_DRIVER})
            if ebs:
                n.volume_limits[EBS_DRIVER] = ebs - 1


def whatif(its, prov, nodes, bound, candidates: List[int], with_cluster_pods: bool = True) -> Problem:
    """simulateScheduling (deprovisioning/helpers.go:42-115): candidate nodes leave the state-node list,
    their pods become the pending batch; the cluster still holds the bound pods (excluded by UID,
    topology.go:66-70,249)."""
    cand = set(candidates)
    ns = [dataclasses.replace(n, in_state=(i not in cand)) for i, n in enumerate(nodes)]
    pods = [p for i in candidates for p in bound[i]]
    # the bound pods only matter to countDomains / inverse anti-affinity; a snapshot whose pods carry no
    # topology terms can skip listing them (nothing would be counted)
    cps = [ClusterPod(uid=p.uid, namespace=p.namespace, node_name=nodes[i].name, labels=p.labels, anti_required=list(p.anti_required))
           for i in range(len(nodes)) for p in bound[i]] if with_cluster_pods else []
    return Problem(instance_types=its, provisioners=[prov], pods=pods, nodes=ns, cluster_pods=cps,
                   extra_well_known=fake.EXTRA_WELL_KNOWN, simulation_mode=True)


def snapshot_problem(its, prov, nodes, bound, with_cluster_pods: bool = True):
    """The whole cluster as ONE problem for `scheduler.open_whatifs`: every node a state node, every bound pod in the pod
    batch (full spec); returns (problem, pod_node).  `whatif()` below builds the same what-if one problem at a time."""
    pods, pod_node = [], []
    for i in range(len(nodes)):
        for p in bound[i]:
            pods.append(p)
            pod_node.append(i)
    ns = [dataclasses.replace(n, in_state=True) for n in nodes]
    cps = [ClusterPod(uid=p.uid, namespace=p.namespace, node_name=nodes[i].name, labels=p.labels, anti_required=list(p.anti_required))
           for i in range(len(nodes)) for p in bound[i]] if with_cluster_pods else []
    return Problem(instance_types=its, provisioners=[prov], pods=pods, nodes=ns, cluster_pods=cps,
                   extra_well_known=fake.EXTRA_WELL_KNOWN, simulation_mode=True), pod_node


def config4_sets(whatifs: int = 512, existing: int = 2048, seed: int = 45) -> List[List[int]]:
    """Candidate sets of config #4: half multi-node prefixes (multinodeconsolidation.go:86-90), half singletons
    (singlenodeconsolidation.go:54)."""
    half = whatifs // 2
    rs = np.random.RandomState(seed + 1)
    return [list(range(0, i + 1)) for i in range(half)] + [[int(rs.randint(existing))] for _ in range(whatifs - half)]


def config4b_snapshot(existing: int = 2048, sizes: int = 50, seed: int = 47):
    """BASELINE configs[3]'s shape over a cluster that is full by pod count: the what-ifs REPLACE (open one node) or fail, instead of all deleting."""
    return cluster_snapshot(existing, sizes, seed, spare_pod_slots=3)      # (a handful of free pod slots in the whole cluster: nearly every what-if opens a node)


def config4(whatifs: int = 512, existing: int = 2048, sizes: int = 50, seed: int = 45, with_cluster_pods: bool = False) -> List[Problem]:
    """512 what-ifs, one Problem each (the per-what-if construction the oracle and the fingerprint tests use)."""
    its, prov, nodes, bound = cluster_snapshot(existing, sizes, seed)
    return [whatif(its, prov, nodes, bound, cs, with_cluster_pods) for cs in config4_sets(whatifs, existing, seed)]


def fresh_node(its, name, rs):
    """An empty owned node of a random instance type / offering of the catalogue, as `cluster_snapshot` makes them (a machine that just joined: cluster.go UpdateNode)."""
    it = its[int(rs.randint(len(its)))]
    off = it.offerings[int(rs.randint(len(it.offerings)))]
    arch = [r for r in it.requirements if r.key == LABEL_ARCH][0].values[0]
    os_ = [r for r in it.requirements if r.key == LABEL_OS][0].values[0]
    labels = {LABEL_PROVISIONER: "default", LABEL_INSTANCE_TYPE: it.name, LABEL_ZONE: off.zone, LABEL_CAPACITY_TYPE: off.capacity_type,
              LABEL_ARCH: arch, LABEL_OS: os_, LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
    return StateNode(name=name, labels=labels, capacity=dict(it.capacity),
                     available={"cpu": f"{int(it.capacity['cpu']) * 1000 - 100}m", "memory": f"{int(it.capacity['memory'][:-2]) * 1024 - 10}Mi", "pods": str(int(it.capacity["pods"]))})


def cluster_after(nodes, bound, events):
    """What a cluster (`cluster_snapshot`'s nodes / per-node bound pods) looks like after `events` (as `model.delta_to_ksd` takes them), the way state.Cluster
    keeps it (cluster.go UpdateNode / DeleteNode / UpdatePod / DeletePod; state/node.go:113,161-182: Available() = Allocatable - the requests of the pods bound):
    returns (nodes, bound, slot) -- fresh lists, removed nodes gone, `slot[i]` = the node's index in the library's snapshot (node slots are never reused: a new
    node takes the next one).  The model the tests hold ParsedProblem.apply against."""
    from .model import format_milli, parse_quantity_milli, pod_requests_milli
    live = [[dataclasses.replace(n, available=dict(n.available)), list(b), i] for i, (n, b) in enumerate(zip(nodes, bound))]
    next_slot = len(nodes)

    def find(name):
        for e in live:
            if e[0].name == name:
                return e
        raise KeyError(name)

    def adjust(n, pod, sign):
        req = pod_requests_milli(pod)
        for k in list(n.available):
            if k in req:
                n.available[k] = format_milli(parse_quantity_milli(n.available[k]) - sign * req[k])

    for ev in events:
        if ev[0] == "node+":
            live.append([dataclasses.replace(ev[1], available=dict(ev[1].available)), [], next_slot])
            next_slot += 1
        elif ev[0] == "node-":
            live.remove(find(ev[1]))
        elif ev[0] == "bind":
            e = find(ev[1])
            adjust(e[0], ev[2], +1)
            e[1].append(ev[2])
        elif ev[0] == "unbind":
            for e in live:
                hit = [p for p in e[1] if p.uid == ev[1]]
                if hit:
                    adjust(e[0], hit[0], -1)
                    e[1].remove(hit[0])
                    break
            else:
                raise KeyError(ev[1])
        elif ev[0] == "node=":      # (the object is replaced -- its values as given, already net of the pods bound; the bound list and the slot stay)
            find(ev[1].name)[0] = dataclasses.replace(ev[1], available=dict(ev[1].available))
    return [e[0] for e in live], [e[1] for e in live], [e[2] for e in live]


# ---- node reconciliations: state.Cluster.UpdateNode for a node that is in state already (the `node=` event) ----
UPDATE_KINDS = ("initialized", "taint", "zone", "available", "volume_limits", "owner")
UPDATE_TAINTS = [Taint("node.example.com/maintenance", "true", NO_SCHEDULE), Taint("node.example.com/dedicated", "batch", NO_SCHEDULE)]


def updated_node(rs, node, kind):
    """`node` -- the object the cluster holds NOW (`cluster_after`'s: available net of the pods bound, usage following them) -- after one reconciliation of `kind`:
    the initialised label flips (true <-> false), a taint of UPDATE_TAINTS is set or cleared, the zone label moves to another of ZONES, available cpu shrinks or
    grows by a few hundred millicores, the CSINode limit of the EBS driver changes, or the provisioner-name label goes / comes back (owned <-> unowned).
    A fresh object: every other field is the node's own."""
    from .model import format_milli
    n = dataclasses.replace(node, labels=dict(node.labels), taints=list(node.taints), available=dict(node.available), volume_limits=dict(node.volume_limits))
    if kind == "initialized":
        n.labels["karpenter.sh/initialized"] = "false" if n.labels.get("karpenter.sh/initialized") == "true" else "true"
    elif kind == "taint":
        t = UPDATE_TAINTS[int(rs.randint(len(UPDATE_TAINTS)))]
        n.taints = [x for x in n.taints if x != t] if t in n.taints else n.taints + [t]
    elif kind == "zone":
        n.labels[LABEL_ZONE] = [z for z in ZONES if z != n.labels.get(LABEL_ZONE)][int(rs.randint(len(ZONES) - 1))]
    elif kind == "available":
        have = parse_quantity_milli(n.available["cpu"])
        n.available["cpu"] = format_milli(max(0, have + int(rs.choice([-700, -300, 200, 500]))))
    elif kind == "volume_limits":
        n.volume_limits[EBS_DRIVER] = int(rs.choice([2, 3, 5, 25, 39]))
    elif kind == "owner":
        if n.labels.get(LABEL_PROVISIONER):
            del n.labels[LABEL_PROVISIONER]
        else:
            n.labels[LABEL_PROVISIONER] = "default"
    else:
        raise ValueError(f"unknown node update {kind!r}")
    return n


def random_events_with_updates(rs, its, nodes, bound, n, tag, removes=True, make_pod=generic_pod, after=cluster_after, new_node=fresh_node, kinds=UPDATE_KINDS, share=0.25):
    """`n` events against the cluster (nodes, bound) as it is, about `share` of them `node=` (a reconciliation of a random live node, of a random kind of
    `kinds`), the others node+ / bind / unbind / node-; returns them with the cluster they lead to (`after`: the model, `cluster_after` or a wrapper of it)."""
    events = []
    for k in range(n):
        if events:
            nodes, bound, _ = after(nodes, bound, events[-1:])
        if rs.rand() < share:
            events.append(("node=", updated_node(rs, nodes[int(rs.randint(len(nodes)))], kinds[int(rs.randint(len(kinds)))])))
            continue
        kind = rs.choice(["node+", "bind", "bind", "bind"] + (["unbind", "unbind", "node-"] if removes else []))
        if kind == "node+":
            events.append(("node+", new_node(its, f"{tag}-node-{k}", rs)))
        elif kind == "node-" and len(nodes) > 4:
            events.append(("node-", nodes[int(rs.randint(len(nodes)))].name))
        elif kind == "unbind" and any(bound):
            i = int(rs.choice([j for j, b in enumerate(bound) if b]))
            events.append(("unbind", bound[i][int(rs.randint(len(bound[i])))].uid))
        else:
            events.append(("bind", nodes[int(rs.randint(len(nodes)))].name, make_pod(rs, f"{tag}-pod-{k}")))
    if events:
        nodes, bound, _ = after(nodes, bound, events[-1:])
    return events, nodes, bound


# ---- catalogue changes: what cloudProvider.GetInstanceTypes answers differently from one pass to the next (the `IT=` event) ----
CATALOGUE_KINDS = ("availability", "price", "pair", "values", "rare")
RARE_ZONE, RARE_OS = "test-zone-9", "plan9"


def with_offerings(it, offerings):
    """`it` with these offerings, its zone / capacity-type requirement values following the available ones (fake/instancetype.go:48-106 and the cloud providers
    derive both from Offerings.Available())."""
    from .model import Expr
    avail = [o for o in offerings if o.available]
    reqs = [Expr(LABEL_ZONE, "In", [o.zone for o in avail]) if r.key == LABEL_ZONE else
            Expr(LABEL_CAPACITY_TYPE, "In", [o.capacity_type for o in avail]) if r.key == LABEL_CAPACITY_TYPE else r for r in it.requirements]
    return dataclasses.replace(it, requirements=reqs, offerings=list(offerings))


def updated_type(rs, it, kind):
    """The instance type `it` as the provider lists it after one change of `kind`: an offering's availability flips, its price moves, a (zone, capacity-type) pair
    is listed or no longer listed, a value joins or leaves the operating-system requirement, or -- `rare` -- something the catalogue has nowhere else comes or
    goes (an offering in RARE_ZONE, the operating system RARE_OS).  A fresh object; name, capacity and overhead are the type's own."""
    from .model import Expr, Offering
    offs = [dataclasses.replace(o) for o in it.offerings]
    if kind == "availability":
        o = offs[int(rs.randint(len(offs)))]
        o.available = not o.available
        return with_offerings(it, offs)
    if kind == "price":
        o = offs[int(rs.randint(len(offs)))]
        o.price = round(o.price * float(rs.choice([0.5, 0.8, 1.25, 2.0])), 6)
        return with_offerings(it, offs)
    if kind == "pair":
        have = {(o.zone, o.capacity_type) for o in offs}
        missing = [(z, c) for z in ZONES for c in ("spot", "on-demand") if (z, c) not in have]
        if missing and (len(offs) < 2 or rs.rand() < 0.5):
            z, c = missing[int(rs.randint(len(missing)))]
            offs.append(Offering(c, z, offs[0].price if offs else 1.0))
        elif len(offs) > 1:
            offs.pop(int(rs.randint(len(offs))))
        return with_offerings(it, offs)
    if kind == "values" or kind == "rare":
        if kind == "rare" and rs.rand() < 0.5:
            if any(o.zone == RARE_ZONE for o in offs):
                offs = [o for o in offs if o.zone != RARE_ZONE]
            else:
                offs.append(Offering("on-demand", RARE_ZONE, offs[0].price if offs else 1.0))
            return with_offerings(it, offs)
        pool = [RARE_OS] if kind == "rare" else ["linux", "windows", "darwin"]
        reqs = []
        for r in it.requirements:
            if r.key == LABEL_OS:
                v = pool[int(rs.randint(len(pool)))]
                vals = [x for x in r.values if x != v] if v in r.values and len(r.values) > 1 else sorted(set(r.values) | {v})
                r = Expr(LABEL_OS, "In", vals)
            reqs.append(r)
        return dataclasses.replace(it, requirements=reqs)
    raise ValueError(f"unknown catalogue change {kind!r}")


def catalogue_after(its, events):
    """The catalogue after the `IT=` events among `events`: every type in its place, the named ones replaced (the model the tests hold `ParsedProblem.apply` against)."""
    out = list(its)
    for ev in events:
        if ev[0] == "IT=":
            out[[t.name for t in out].index(ev[1].name)] = ev[1]
    return out


def random_events_with_catalogue(rs, its, nodes, bound, n, tag, share=0.3, changes=CATALOGUE_KINDS, **kw):
    """`n` events, `share` of them `IT=` (a change of a random kind of `changes` to a random type of the catalogue as it is now), the others
    `random_events_with_updates`' (`kw` goes there); returns (events, catalogue, nodes, bound) as they are after the events.  Nodes that join are of the ORIGINAL types (a node may carry any label)."""
    n_cat = int(round(n * share))
    other, nodes2, bound2 = random_events_with_updates(rs, its, nodes, bound, n - n_cat, tag, **kw)
    events, cat = [], list(its)
    at = sorted(int(x) for x in rs.randint(0, len(other) + 1, size=n_cat))      # (the catalogue events go in between the others; both kinds keep their order)
    for k in range(len(other) + 1):
        for _ in range(at.count(k)):
            t = int(rs.randint(len(cat)))
            cat[t] = updated_type(rs, cat[t], changes[int(rs.randint(len(changes)))])
            events.append(("IT=", cat[t]))
        events += other[k:k + 1]
    return events, cat, nodes2, bound2


# ---- a cloud-like catalogue with 9 to 16 resource names ----
# The names an AWS-style provider lists on every instance type, whether or not the type has the device, then what device plugins add.
WIDE_NAMES = ["cpu", "memory", "ephemeral-storage", "pods", "vpc.amazonaws.com/pod-eni", "nvidia.com/gpu", "amd.com/gpu", "aws.amazon.com/neuron",
              "habana.ai/gaudi", "hugepages-2Mi", "vpc.amazonaws.com/efa", "hugepages-1Gi", "xilinx.com/fpga", "example.com/nic", "smarter-devices/fuse",
              "intel.com/qat"]
GPU_TAINT = Taint("nvidia.com/gpu", "true", NO_SCHEDULE)


def wide_requested(names: int) -> List[str]:
    """The names something in `wide_catalogue(names=...)` requests, limits or consumes (at most 8); the others only ever appear in a catalogue or a node's capacity."""
    return WIDE_NAMES[:6] + [n for n in ("hugepages-2Mi", "vpc.amazonaws.com/efa") if n in WIDE_NAMES[:names]]


def wide_catalogue(names: int = 9, pods: int = 400, types: int = 24, existing: int = 6, seed: int = 0, strip: bool = False, dense: bool = False) -> Problem:
    """A provisioning Solve over a catalogue whose instance types list `names` (9..16) resource names, most of them 0 on most types: general-purpose
    sizes, GPU types behind a tainted provisioner with a limit on nvidia.com/gpu (subtractMax / filterByRemainingResources over the wide vector), existing
    nodes whose `available` carries the extended names, a daemonset requesting ephemeral-storage, and pods that request subsets of the names -- some
    through limits only, some through init containers -- with zonal spread and preferences that relax.
    strip=True: the same problem with every name that nothing requests removed from the catalogue and the nodes (R <= 8: today's kernels).
    dense=True (names >= 12): the same problem with requests on every name of the catalogue, so that resources 8.. are requested too (`_densify`)."""
    assert 9 <= names <= len(WIDE_NAMES) and not (strip and dense) and (names >= 12 or not dense)
    rs = np.random.RandomState(9000 + seed)
    catalogue = WIDE_NAMES[:names]
    keep = set(wide_requested(names)) if strip else set(catalogue)
    hp, efa = "hugepages-2Mi" in catalogue, "vpc.amazonaws.com/efa" in catalogue
    its, gpu_idx = [], []
    for i in range(types):
        gpu = i % 4 == 3
        cpu = [2, 4, 8, 16, 32, 48, 64, 96][int(rs.randint(8))]
        cap = {n: "0" for n in catalogue}
        cap.update({"cpu": str(cpu), "memory": f"{cpu * int(rs.choice([2, 4, 8]))}Gi", "ephemeral-storage": f"{int(rs.choice([20, 100, 500]))}Gi",
                    "pods": str(int(rs.choice([29, 58, 110, 234]))), "vpc.amazonaws.com/pod-eni": str(int(rs.choice([0, 9, 38, 107])))})
        if gpu:
            cap["nvidia.com/gpu"] = str(int(rs.choice([1, 2, 4, 8])))
            if efa:
                cap["vpc.amazonaws.com/efa"] = str(int(rs.choice([0, 1, 4])))
        elif rs.rand() < 0.2:
            cap[["amd.com/gpu", "aws.amazon.com/neuron", "habana.ai/gaudi"][int(rs.randint(3))]] = str(int(rs.choice([1, 4, 16])))
        if hp and cpu >= 8:
            cap["hugepages-2Mi"] = f"{int(rs.choice([0, 512, 2048]))}Mi"
        for n in catalogue[11:]:
            if rs.rand() < 0.3:
                cap[n] = str(int(rs.randint(1, 8)))
        it = fake.new_instance_type(f"{'g' if gpu else 'm'}{i:03d}-{cpu}x", resources={k: v for k, v in cap.items() if k in keep},
                                    architecture="amd64", operating_systems=["linux"])
        it.overhead = {"cpu": "100m", "memory": "10Mi", "ephemeral-storage": "1Gi"}
        its.append(it)
        if gpu:
            gpu_idx.append(i)
    gen = [i for i in range(types) if i not in gpu_idx]
    provs = [fake.provisioner("gpu", weight=10, taints=[GPU_TAINT], instance_types=gpu_idx,
                              limits={"nvidia.com/gpu": str(int(rs.randint(8, 48))), "cpu": str(int(rs.randint(200, 800)))}),
             fake.provisioner("default", instance_types=gen, limits={"cpu": str(int(rs.randint(pods // 2 + 2, 2 * pods + 3)))} if rs.rand() < 0.5 else None)]
    nodes = []
    for e in range(existing):
        ti = int(rs.randint(types))
        it = its[ti]
        frac = rs.uniform(0.2, 0.9)
        avail = {}
        for n, v in it.capacity.items():
            m = parse_quantity_milli(v)
            avail[n] = str(int(m * frac) // 1000) if n in ("cpu", "pods") or n not in ("memory", "ephemeral-storage", "hugepages-2Mi") else f"{int(m * frac) // 1000 // 2**20}Mi"
        zone = it.offerings[int(rs.randint(len(it.offerings)))]
        name = f"wide-node-{e:04d}"
        labels = {LABEL_PROVISIONER: "gpu" if ti in gpu_idx else "default", LABEL_INSTANCE_TYPE: it.name, LABEL_ZONE: zone.zone,
                  LABEL_CAPACITY_TYPE: zone.capacity_type, LABEL_ARCH: "amd64", LABEL_OS: "linux", LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
        nodes.append(StateNode(name=name, labels=labels, taints=[GPU_TAINT] if ti in gpu_idx else [], available=avail, capacity=dict(it.capacity)))
    out = []
    for k in range(pods):
        c = Container(requests={"cpu": f"{CPU_CHOICES[rs.randint(len(CPU_CHOICES))]}m", "memory": f"{MEM_CHOICES[rs.randint(len(MEM_CHOICES))]}Mi"})
        p = Pod(uid=f"wide-{k:06d}", labels={"my-label": _lab(rs)}, containers=[c])
        kind = int(rs.randint(10))
        if kind == 0:
            c.requests["ephemeral-storage"] = f"{int(rs.choice([1, 4, 30]))}Gi"
        elif kind == 1:
            c.limits["vpc.amazonaws.com/pod-eni"] = "1"                      # limits only: the request defaults to the limit
        elif kind in (2, 3):
            c.limits["nvidia.com/gpu"] = str(int(rs.choice([1, 1, 2, 4])))
            if kind == 3 and efa:
                c.limits["vpc.amazonaws.com/efa"] = "1"
            p.tolerations = [Toleration(key=GPU_TAINT.key, operator="Exists")]
        elif kind == 4:
            init = Container(requests={"cpu": f"{int(rs.choice([500, 2000, 6000]))}m"})
            if hp:
                init.requests["hugepages-2Mi"] = f"{int(rs.choice([64, 256]))}Mi"
            p.init_containers = [init]
        elif kind == 5:
            p.preferred_affinity = [PreferredTerm(10, [Expr(LABEL_ZONE, "In", ["no-such-zone"])]), PreferredTerm(5, [Expr(LABEL_CAPACITY_TYPE, "In", ["spot"])])]
        elif kind == 6:
            p.spread = [TopologySpreadConstraint(1, LABEL_ZONE, DO_NOT_SCHEDULE, LabelSelector({"my-label": p.labels["my-label"]}))]
        elif kind == 7 and rs.rand() < 0.3:
            c.requests["cpu"] = "200"                                         # fits nothing: stays unschedulable
        out.append(p)
    ds = [Pod(uid="wide-ds", containers=[Container(requests={"cpu": "50m", "memory": "32Mi", "ephemeral-storage": "512Mi"})])]
    pr = Problem(instance_types=its, provisioners=provs, pods=out, daemonset_pods=ds, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)
    return _densify(pr, catalogue, seed) if dense else pr


# device names the general-purpose (untainted) types may carry, and the unit a request of each is written in
_DENSE_DEVICES = {"amd.com/gpu": "", "aws.amazon.com/neuron": "", "habana.ai/gaudi": "", "hugepages-2Mi": "Mi", "hugepages-1Gi": "", "xilinx.com/fpga": "",
                  "example.com/nic": "", "smarter-devices/fuse": "", "intel.com/qat": ""}


def _densify(pr: Problem, catalogue: List[str], seed: int) -> Problem:
    """wide_catalogue(dense=True): requests on resources 8.. of the encoding (cpu, memory, pods, then first use -- the first provisioner's limits
    name every catalogue name, so the order is the sorted catalogue).  The GPU provisioner's limit on nvidia.com/gpu and the default provisioner's
    limits on two late names bind; pods request devices through requests, limits only and init containers; pairs of pods differ only in a request
    on a late name (distinct evaluation classes); existing nodes hold one or two of a late device; a second daemonset, on the GPU provisioner's
    nodes only, requests vpc.amazonaws.com/efa.  Its own random stream: the problem it starts from is wide_catalogue(dense=False)'s."""
    rd = np.random.RandomState(19000 + seed)
    order = ["cpu", "memory", "pods"] + sorted(n for n in catalogue if n not in ("cpu", "memory", "pods"))
    late = [n for n in order[8:] if n in _DENSE_DEVICES]
    gpu, default = pr.provisioners
    gpu.limits = dict({n: "1000000Gi" for n in catalogue}, **gpu.limits)
    def limit(n):      # what the existing nodes of the provisioner hold (remainingResources starts below it), plus room for a few new nodes
        held = sum(parse_quantity_milli(nd.capacity.get(n, "0")) for nd in pr.nodes if nd.labels.get(LABEL_PROVISIONER) == "default") // 1000
        return f"{held // 2**20 + int(rd.randint(30, 120)) * 1024}Mi" if _DENSE_DEVICES[n] else str(held + int(rd.randint(30, 120)))
    default.limits = dict(default.limits or {}, **{n: limit(n) for n in late[:2]})
    for it in pr.instance_types:
        if it.name.startswith("m") and rd.rand() < 0.6:
            for n in rd.choice(sorted(_DENSE_DEVICES.keys() & set(catalogue)), size=2, replace=False):
                it.capacity[n] = f"{int(rd.choice([512, 2048]))}Mi" if _DENSE_DEVICES[n] else str(int(rd.randint(1, 6)))
    for nd in pr.nodes:
        for n in late:
            if n in nd.available and nd.available[n] != "0":
                nd.available[n] = str(int(rd.randint(1, 3)))
    devices = sorted(_DENSE_DEVICES.keys() & set(catalogue))
    for p in pr.pods:
        if p.tolerations or p.containers[0].requests.get("cpu") == "200" or rd.rand() < 0.5:
            continue
        n = devices[int(rd.randint(len(devices)))]
        q = f"{int(rd.choice([64, 256]))}Mi" if _DENSE_DEVICES[n] else str(int(rd.choice([1, 1, 2])))
        how = int(rd.randint(3))
        if how == 0:
            p.containers[0].requests[n] = q
        elif how == 1:
            p.containers[0].limits[n] = q                                 # limits only
        else:
            p.init_containers = [Container(requests={"cpu": "100m", n: q})]
    for k, n in enumerate(late[:3]):                                          # same spec but for a request on a late name
        for amount in ("1", "2"):
            pr.pods.append(Pod(uid=f"wide-pair-{k}-{amount}", labels={"my-label": "pair"},
                               containers=[Container(requests={"cpu": "250m", "memory": "256Mi", n: amount})]))
    pr.daemonset_pods = pr.daemonset_pods + [Pod(uid="wide-ds-gpu", node_selector={LABEL_PROVISIONER: "gpu"}, tolerations=[Toleration(key=GPU_TAINT.key, operator="Exists")],
                                                 containers=[Container(requests={"cpu": "10m", "vpc.amazonaws.com/efa": "1"})])]
    return pr


# ---- any problem dressed in a cloud provider's catalogue ----
# names 17.. of a dressing: what further device plugins add (WIDE_NAMES stops at the 16 the wide kernels hold)
CLOUD_EXTRA_NAMES = ["gpu.intel.com/i915", "squat.ai/video", "devices.kubevirt.io/kvm", "example.com/dongle", "example.com/tpm", "example.com/sgx-epc"]


def cloud_catalogue(problem: Problem, names: int = 12, seed: int = 0) -> Problem:
    """A deep copy of `problem` whose instance types and state nodes all list the first `names` (up to 22) of WIDE_NAMES + CLOUD_EXTRA_NAMES, the way a cloud
    provider's catalogue does: a name a type or node already carries keeps its quantity, every other one is added -- 0 on most types (`wide_catalogue` does the
    same), a few devices on some; a node gets the added names in `capacity` and `available` alike.  Pods, daemonsets and provisioners are untouched, so the
    added names are requested and limited by nothing unless the problem already did: every decision is the undressed problem's."""
    import copy
    pool = WIDE_NAMES + CLOUD_EXTRA_NAMES
    assert 1 <= names <= len(pool)
    rs = np.random.RandomState(29000 + seed)
    pr = copy.deepcopy(problem)
    for it in pr.instance_types:
        for n in pool[:names]:
            if n not in it.capacity:
                it.capacity[n] = str(int(rs.choice([1, 2, 4, 8]))) if rs.rand() < 0.15 else "0"
    for nd in pr.nodes:
        for n in pool[:names]:
            q = str(int(rs.choice([1, 2]))) if rs.rand() < 0.15 else "0"
            if n not in nd.capacity:
                nd.capacity[n] = q
            if n not in nd.available:
                nd.available[n] = q if nd.capacity[n] == q else "0"
    return pr
