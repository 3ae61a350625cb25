"""Problems for ks_pack_rr's RUN rounds over stretches of plain replicas longer than one 64-lane chunk of the queue (RR_RUN_MAX), shared by
tests/test_rr_long_runs.py (lane-fibre emulator) and tests/test_rr_long_runs_gpu.py.

A RUN round places the pods of a step on the nodes of ONE count bucket, so a stretch only stays with RUN rounds (RR_RUN_KEEP: three pods a step on average) while
several nodes stand side by side.  Every problem therefore starts with `openers` pods that each need a machine of their own (self-selecting hostname
anti-affinity, larger requests: they sort first); the replicas behind them go round those machines, `openers` pods a step.  All LEAN, one instance type."""
from karpenter_core_amd import fake
from karpenter_core_amd.model import (Container, DO_NOT_SCHEDULE, Expr, LABEL_ARCH, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_OS, LABEL_PROVISIONER,
                                      LABEL_ZONE, LabelSelector, Pod, PodAffinityTerm, PreferredTerm, Problem, StateNode, TopologySpreadConstraint)

OPENERS = 40


def _box(pods_per_node):
    return fake.new_instance_type("box", {"cpu": "64", "memory": "256Gi", "pods": str(pods_per_node)})


def _opener(i):
    return Pod(uid=f"a-open-{i:05d}", labels={"role": "opener"}, containers=[Container(requests={"cpu": "1000m", "memory": "512Mi"})],
               anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"role": "opener"}))])


def _replica(i, labels=None, **kw):
    return Pod(uid=f"r-web-{i:05d}", labels=dict({"app": "web"}, **(labels or {})), containers=[Container(requests={"cpu": "100m", "memory": "64Mi"})], **kw)


def _problem(its, pods, nodes=()):
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=pods, nodes=list(nodes), extra_well_known=fake.EXTRA_WELL_KNOWN)


def stretch(replicas, openers=OPENERS, per_node=160):
    """`openers` machines, then ONE stretch of `replicas` identical plain replicas (a node holds the opener and per_node - 1 replicas)."""
    return _problem([_box(per_node)], [_opener(i) for i in range(openers)] + [_replica(i) for i in range(replicas)])


def stretch_then_other_class(length, tail=100):
    """The stretch ends after `length` replicas: behind it `tail` replicas of ANOTHER base class (other requests, sorted behind: less memory)."""
    pods = [_opener(i) for i in range(OPENERS)] + [_replica(i) for i in range(length)]
    pods += [Pod(uid=f"s-api-{i:05d}", labels={"app": "api"}, containers=[Container(requests={"cpu": "100m", "memory": "32Mi"})]) for i in range(tail)]
    return _problem([_box(160)], pods)


def full_machines(fill, holds, more=90):
    """Every machine holds `holds` replicas beside its opener; the machines are full after `fill` replicas (fillers -- replicas of another base class that sort in
    front -- take the slots that `fill` leaves over), and the stretch goes on for `more` pods: the pod that needs a NEW machine is entry `fill` of the stretch."""
    openers = (fill + holds - 1) // holds
    fillers = openers * holds - fill
    pods = [_opener(i) for i in range(openers)]
    pods += [Pod(uid=f"b-fill-{i:05d}", labels={"app": "fill"}, containers=[Container(requests={"cpu": "100m", "memory": "128Mi"})]) for i in range(fillers)]
    pods += [_replica(i) for i in range(fill + more)]
    return _problem([_box(1 + holds)], pods)


def hostname_groups(first, groups=30, size=5, names=12, lead=12, both=False):
    """Replicas of one base class whose hostname-keyed items DIFFER, behind `lead` plain ones (RUN rounds start on those): every `size` pods in a row (the first
    group: `first`) form a group of their own, in turn one under a self-selecting hostname anti-affinity and one under a hostname spread over the group -- a step
    of a run ends where the items change.  both: every pod carries a hostname spread over the deployment AND its group's anti-affinity (three hostname-keyed
    items with the term's inverse: past what a base class holds, every group is a run of its own).  (`names` group labels, taken in turn: the kernel keeps 32
    hostname-keyed counters per node, and every anti-affinity term brings its inverse group.)"""
    pods = [_opener(i) for i in range(OPENERS)] + [_replica(i) for i in range(lead)]
    i = lead
    for g in range(groups):
        grp = f"g{g % names:02d}"
        anti = [PodAffinityTerm(LABEL_HOSTNAME, LabelSelector({"grp": grp}))]
        if both:
            kw = {"anti_required": anti, "spread": [TopologySpreadConstraint(64, LABEL_HOSTNAME, DO_NOT_SCHEDULE, LabelSelector({"app": "web"}))]}
        else:
            kw = {"anti_required": anti} if g % 2 == 0 else {"spread": [TopologySpreadConstraint(2, LABEL_HOSTNAME, DO_NOT_SCHEDULE, LabelSelector({"grp": grp}))]}
        for _ in range(first if g == 0 else size):
            pods.append(_replica(i, labels={"grp": grp}, **kw))
            i += 1
    return _problem([_box(160)], pods)


def requeued_inside_a_stretch(before, after=150, openers=7):
    """A replica with a preferred node-affinity term nothing meets: it fails where it stands (`before` replicas in front of it), is relaxed and pushed to the tail of
    the queue -- a plain replica of the stretch's base class now, behind `after` more of them; and, last in the queue, one replica no machine takes (its zone does
    not exist): it fails for good and is requeued UNRELAXED behind that.  (Seven machines: the kernel gives a Solve back -- decline 3 -- when the exact filter
    refuses a pod on more than eight nodes.)"""
    pods = [_opener(i) for i in range(openers)] + [_replica(i) for i in range(before)]
    pods.append(_replica(before, preferred_affinity=[PreferredTerm(10, [Expr(LABEL_ZONE, "In", ["no-such-zone"])])]))
    pods += [_replica(before + 1 + i) for i in range(after)]
    pods.append(_replica(before + 1 + after, node_selector={LABEL_ZONE: "no-such-zone"}))
    return _problem([_box(160)], pods)


def existing_nodes(replicas=300, existing=40, free=3):
    """The stretch with `existing` in-flight nodes that have `free` pod slots each (one goes to an opener; the other openers open machines): the run starts on
    existing nodes (an existing node ends a step) and goes on over the machines."""
    it = _box(160)
    nodes = []
    for e in range(existing):
        name = f"node-{e:05d}"
        labels = {LABEL_PROVISIONER: "default", LABEL_INSTANCE_TYPE: it.name, LABEL_ZONE: "test-zone-1", LABEL_CAPACITY_TYPE: "on-demand", LABEL_ARCH: "amd64",
                  LABEL_OS: "linux", LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
        nodes.append(StateNode(name=name, labels=labels, available={"cpu": "8000m", "memory": "32768Mi", "pods": str(free)}, capacity=dict(it.capacity)))
    return _problem([it], [_opener(i) for i in range(existing + OPENERS)] + [_replica(i) for i in range(replicas)], nodes)


# name -> (maker, meant to be long: the average run is longer than 64 pods in a build whose RR_RUN_MAX is)
EDGES = [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]
CASES = {"stretch_300": (lambda: stretch(300), True)}
# the head window keeps the first HEAD plain replicas (RR_WIN_PLAIN ends its phase at the eighth) before RUN rounds take over: a stretch of HEAD + n ends at run-relative entry n
HEAD = 7
for n in EDGES:
    CASES[f"ends_at_{n}"] = (lambda n=n: stretch_then_other_class(HEAD + n), n > 70)
for holds in (7, 8, 9):
    for at in (64, 96, 128):                       # the new machine at a chunk boundary, in the middle of a chunk, at the next boundary
        CASES[f"full_{holds}_at_{at}"] = (lambda holds=holds, at=at: full_machines(HEAD + at, holds), False)
for first in (1, 2, 3, 4, 5):                      # the items change every 5 entries, from `first` on: at and next to entries 64 and 128 of the run for one `first` or another
    CASES[f"groups_first_{first}"] = (lambda first=first: hostname_groups(first), True)
CASES["groups_both_3"] = (lambda: hostname_groups(3, both=True), False)
CASES["requeued_60"] = (lambda: requeued_inside_a_stretch(60), True)
CASES["requeued_200"] = (lambda: requeued_inside_a_stretch(200), True)
CASES["existing_40"] = (lambda: existing_nodes(), True)
