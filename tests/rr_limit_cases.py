"""Problems that stand at the LAST value each of ks_pack_rr's fixed-size tables and packed fields takes, and at the first one past it (csrc/ks_pack_rr.inc:35-45: what
the kernel covers and the decline codes; DESIGN 7.13a lists limit, constant, code and case), shared by tests/test_rr_limits.py (the kernel's source on the lane-fibre
emulator) and tests/test_rr_limits_gpu.py.  All LEAN, R <= 4, small.

CASES: name -> (maker, expected rr_status() as (started, code), family, rung).  (1, 0): ks_pack_rr took the Solve and kept it.  Within a family the taken rungs are a
prefix in rung order and both sides of the boundary are there; the families of TAKEN_ONLY have taken rungs only (they pin what must NOT trip a limit).

What is not here, and why:
  code 6 (an anti-affinity group that does not exist yet when a machine is opened, ks_pack_rr.inc try_open: `else if (!act) { hok = false; err = 6; }`) cannot be
      reached through FlatProblem: the item must be of type 2 (type 1 makes the class `bad`, code 7, in ks_build_rr), every anti-affinity term of a pod's FIRST stage
      creates its group active (host/encode.cpp: `stages[0].sg = groups_of(spec, true)`), a type-2 group's identity has no node filter, and Preferences.Relax only
      REMOVES terms -- a later stage owns no anti-affinity group the first did not.  (Only spread groups are created late: their identity carries the node filter,
      which changes when a required node-affinity term is dropped; those take the `ty == 0` arm, a plain topology refusal.)
  code 9 (`else if (nnew >= nMAX) err = 9` in try_open) cannot be reached either: the flattening sets max_new_nodes = P (host/encode.cpp: `p.max_new_nodes = p.P ? p.P
      : 1`), a machine is opened only for a pod that is then committed to it, so with nnew == P every pod is placed and nothing asks for another machine.
  code 8 is the round watchdog: a protocol bug, not a size.
  the pod count (RR_SEQMAX, 524 287): building half a million pod objects is not a test of a few seconds.
  a pod with FOUR hostname-keyed items: refused by the flattening (Unsupported) before any kernel -- one assertion in the test modules (UNSUPPORTED below), not a case."""
import hashlib
import json
import random

import long_runs_cases as LC
from karpenter_core_amd import fake
from karpenter_core_amd.model import (Container, DO_NOT_SCHEDULE, Expr, LABEL_ARCH, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_OS, LABEL_PROVISIONER,
                                      LABEL_ZONE, LabelSelector, Pod, PodAffinityTerm, Problem, StateNode, TopologySpreadConstraint)

ZONES = ["test-zone-1", "test-zone-2", "test-zone-3"]
TEAM = "example.com/team"
TAKEN = (1, 0)


def _pod(uid, cpu="10m", mem="8Mi", extra=None, **kw):
    return Pod(uid=uid, containers=[Container(requests=dict({"cpu": cpu, "memory": mem}, **(extra or {})))], **kw)


def _tiny(n, **kw):
    return [_pod(f"z-tiny-{i:05d}", **kw) for i in range(n)]


def _problem(its, pods, nodes=(), provisioners=None):
    return Problem(instance_types=its, provisioners=provisioners or [fake.provisioner("default", len(its))], pods=pods, nodes=list(nodes), extra_well_known=fake.EXTRA_WELL_KNOWN)


def _spread(key, labels, skew=1):
    return TopologySpreadConstraint(skew, key, DO_NOT_SCHEDULE, LabelSelector(dict(labels)))


def _state_nodes(it, count, available, zones=ZONES[:1], capacity_types=("on-demand",)):
    """In-flight nodes of type `it` (the recipe of long_runs_cases.existing_nodes), dealt over `zones` and `capacity_types` in turn."""
    nodes = []
    for e in range(count):
        name = f"node-{e:05d}"
        labels = {LABEL_PROVISIONER: "default", LABEL_INSTANCE_TYPE: it.name, LABEL_ZONE: zones[e % len(zones)], LABEL_CAPACITY_TYPE: capacity_types[(e // len(zones)) % len(capacity_types)],
                  LABEL_ARCH: "amd64", LABEL_OS: "linux", LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
        nodes.append(StateNode(name=name, labels=labels, available=dict(available), capacity=dict(it.capacity)))
    return nodes


# ---- RR_CNTMAX: the count field of a node's key ----
def count_field(capacity, pods=1300):
    """One type that holds `capacity` pods, more tiny pods than that: the first machine fills to its capacity."""
    return _problem([fake.new_instance_type("huge", {"cpu": "4000", "memory": "4000Gi", "pods": str(capacity)})], _tiny(pods))


def count_field_existing(pods):
    """One in-flight node with 1 100 free pod slots: an existing node's key is its index, it has no count field to outgrow."""
    it = fake.new_instance_type("huge", {"cpu": "4000", "memory": "4000Gi", "pods": "500"})
    return _problem([it], _tiny(pods), _state_nodes(it, 1, {"cpu": "3000", "memory": "3000Gi", "pods": "1100"}))


# ---- a_excl[8]: the nodes the exact filter refused for the pod at the head of the queue ----
def exact_filter(n, wide=1, wide_memory="32Gi"):
    """n machines with a 15-cpu pod each (cpu-box or mem-box until the filter says: per resource the maximum of the two, no one type holds both maxima); `wide`
    pods of much memory pass every such node's per-resource screen and fail its exact filter."""
    its = [fake.new_instance_type("cpu-box", {"cpu": "16", "memory": "4Gi", "pods": "32"}), fake.new_instance_type("mem-box", {"cpu": "2", "memory": "64Gi", "pods": "32"})]
    pods = [_pod(f"a-cpu-{i:03d}", "15", "1Gi") for i in range(n)] + [_pod(f"b-wide-{i:03d}", "500m", wide_memory) for i in range(wide)] + _tiny(20)
    return _problem(its, pods)


# ---- RR_NRC: the table of node requirement classes ----
def _team_provisioner(n_types, teams=30):
    return [fake.provisioner("default", n_types, requirements=[Expr(TEAM, "In", [f"t{t:02d}" for t in range(teams)])])]


def nrc_selectors(k):
    """k distinct (team, zone) node selectors, three pods each: every selector is a requirement class of its own."""
    its = fake.instance_types(5)
    combos = [(t, z) for t in range(30) for z in ZONES][:k]
    pods = [_pod(f"s-{t:02d}-{zi}-{j}", "100m", "64Mi", node_selector={TEAM: f"t{t:02d}", LABEL_ZONE: z}) for zi, (t, z) in enumerate(combos) for j in range(3)]
    return _problem(its, pods, provisioners=_team_provisioner(len(its)))


def nrc_children(t):
    """t teams; per team seven pods under the team's selector and a zonal spread over the team's label (a class per team and, narrowed by the spread, a child per
    zone: the highest rows of the dyn1 tables), and 100 tiny pods dealt over the teams."""
    its = fake.instance_types(5)
    pods = []
    for team in range(t):
        lab = {"team": f"t{team:02d}"}
        pods += [_pod(f"s-{team:02d}-{j}", "100m", "64Mi", labels=lab, node_selector={TEAM: f"t{team:02d}"}, spread=[_spread(LABEL_ZONE, lab)]) for j in range(7)]
    pods += [_pod(f"z-tiny-{i:05d}", node_selector={TEAM: f"t{i % t:02d}"}) for i in range(100)]
    return _problem(its, pods, provisioners=_team_provisioner(len(its)))


# ---- G <= 64 groups (bit 63 of tmask_n / rmask_n / g_active_mask), GH <= 32 hostname-keyed groups (hostname slot 31) ----
def _deployments(g, key, size=3, skew=1, first=0):
    pods = []
    for d in range(first, first + g):
        lab = {"app": f"d{d:02d}"}
        pods += [_pod(f"d-{d:02d}-{j:03d}", "100m", "64Mi", labels=lab, spread=[_spread(key, lab, skew)]) for j in range(size)]
    return pods


def zonal_groups(g):
    return _problem(fake.instance_types(5), _deployments(g, LABEL_ZONE))


def zonal_crowd():
    """64 zonal groups; the last two (bits 62 and 63) have 60 pods each, at maxSkew 1 and 2."""
    pods = _deployments(62, LABEL_ZONE) + _deployments(1, LABEL_ZONE, 60, 1, first=62) + _deployments(1, LABEL_ZONE, 60, 2, first=63) + _tiny(150)
    return _problem(fake.instance_types(5), pods)


def _herds(a, size=40):
    """`a` herds of `size` pods under a self-selecting hostname anti-affinity: every term brings its group AND the inverse group."""
    pods = []
    for h in range(a):
        lab = {"herd": f"h{h:02d}"}
        pods += [_pod(f"h-{h:02d}-{j:03d}", "100m", "64Mi", labels=lab, anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector(dict(lab)))]) for j in range(size)]
    return pods


def hostname_groups(g, herds=0):
    return _problem(fake.instance_types(5), _deployments(g, LABEL_HOSTNAME) + _herds(herds))


# ---- K <= 16 keys ----
def keys(j, pods=60):
    """j custom provisioner labels; pod i selects label i mod j (one key per pod: the flattening's 12-keys-per-pod limit stays out of the way)."""
    its = fake.instance_types(5)
    prov = fake.provisioner("default", len(its), labels={f"example.com/k{i:02d}": "v" for i in range(j)})
    return _problem(its, [_pod(f"k-{i:04d}", "100m", "64Mi", node_selector={f"example.com/k{i % j:02d}": "v"}) for i in range(pods)], provisioners=[prov])


# ---- TW <= 128 type words; the Allocatable ladders in dynamic LDS ----
def type_words(T):
    its = [fake.new_instance_type(f"t{i:05d}", {"cpu": str(2 + i % 7), "memory": f"{4 + i % 5}Gi", "pods": "20"}) for i in range(T)]
    return _problem(its, _tiny(100) + _deployments(1, LABEL_ZONE, 9))


def ladders(D):
    """D types with D distinct capacities: R ladders of D rungs each."""
    its = [fake.new_instance_type(f"t{i:05d}", {"cpu": str(1 + i), "memory": f"{1 + i}Gi", "pods": "110"}) for i in range(D)]
    return _problem(its, _tiny(100))


# ---- RR_MAXHREC / RR_MAXNREC: the groups Topology.Record visits for one class; three hostname items; maxSkew 250 ----
def records(n, key):
    """n spreads on `key` over selectors lNN=v, three pods each, and 30 pods that carry ALL n labels: placing one of those records into n groups."""
    pods = []
    for i in range(n):
        lab = {f"l{i:02d}": "v"}
        pods += [_pod(f"d-{i:02d}-{j}", "100m", "64Mi", labels=lab, spread=[_spread(key, lab)]) for j in range(3)]
    every = {f"l{i:02d}": "v" for i in range(n)}
    pods += [_pod(f"e-all-{i:03d}", "50m", "32Mi", labels=every) for i in range(30)]
    return _problem(fake.instance_types(5), pods)


def hostname_items(n, pods=6):
    """Pods with n hostname spreads each (over n labels they all carry)."""
    lab = {f"l{i}": "v" for i in range(n)}
    return _problem(fake.instance_types(5), [_pod(f"i-{j:03d}", "100m", "64Mi", labels=lab, spread=[_spread(LABEL_HOSTNAME, {f"l{i}": "v"}, 1 + i) for i in range(n)]) for j in range(pods)])


def hostname_skew(skew):
    lab = {"app": "web"}
    return _problem(fake.instance_types(5), [_pod(f"w-{j:03d}", "100m", "64Mi", labels=lab, spread=[_spread(LABEL_HOSTNAME, lab, skew)]) for j in range(40)])


# ---- nE <= 64 existing nodes, RR_NODES = 3 584 nodes, node 448 = the first of register slot 1 ----
def one_pod_machines(existing, new, tiny=600):
    """`existing` in-flight nodes with three free pod slots and existing + new openers (self-selecting hostname anti-affinity: a node each), then `tiny` replicas."""
    it = LC._box(160)
    nodes = _state_nodes(it, existing, {"cpu": "8000m", "memory": "32768Mi", "pods": "3"})
    return _problem([it], [LC._opener(i) for i in range(existing + new)] + [LC._replica(i) for i in range(tiny)], nodes)


def node_count(n):
    """n pods that need a machine each and nothing else."""
    lab = {"app": "x"}
    its = fake.instance_types(5)
    return _problem(its, [_pod(f"pod-{i:07d}", "100m", "64Mi", labels=lab, anti_required=[PodAffinityTerm(LABEL_HOSTNAME, LabelSelector(dict(lab)))]) for i in range(n)])


# ---- pod_reason holds eight nibbles: templates beyond it ----
def templates(m):
    """m provisioners, all restricted to zone 1; pods that ask for zone 2 (every template refuses: requirements) and pods no type holds; some that fit."""
    its = fake.instance_types(5)
    provs = [fake.provisioner(f"p{i:02d}", len(its), requirements=[Expr(LABEL_ZONE, "In", [ZONES[0]])]) for i in range(m)]
    pods = [_pod(f"a-zone2-{i}", "100m", "64Mi", node_selector={LABEL_ZONE: ZONES[1]}) for i in range(4)] + [_pod(f"b-large-{i}", "1000", "64Mi") for i in range(4)] + _tiny(30)
    return _problem(its, pods, provisioners=provs)


# ---- everything at once ----
COMBINED_KEYS = 13      # custom provisioner labels: K = 16 with the three keys every problem has


def combined(custom_keys=COMBINED_KEYS, seed=25, split=False):
    """64 in-flight nodes over three zones and two capacity types, 32 zonal and 32 hostname groups (G counts both: 64) with a crowd on the last of each, a fourth
    resource requested by a tenth of the pods, 150 plain pods, in a seeded shuffle.  `custom_keys` provisioner labels, each selected by some PLAIN pods.
    The host-side gate that refuses this shape once labels are added to ALL its pods is `q.G > KS_FAST_G` (ksolve.hip, the batch's traits in front of the launch of
    ks_pack_rr: `fast`): a spread's node filter (MakeTopologyNodeFilter: the owner's node selector) is part of its group's identity, so a deployment whose pods select
    different labels is one group per label and G leaves 64 -- ks_pack_rr is never launched, (0, 0).  split: the crowd of the last zonal deployment selects one of
    two labels in turn (G = 65).  The gate says nothing about keys; those are the kernel's own K <= 16, and plain pods may use all thirteen."""
    gpu = fake.RES_GPU_A
    its = [fake.new_instance_type(f"box-{i}", {"cpu": str(8 * (i + 1)), "memory": f"{32 * (i + 1)}Gi", "pods": "60", gpu: str(4 * (i + 1))}) for i in range(4)]
    nodes = _state_nodes(its[1], 64, {"cpu": "4000m", "memory": "16384Mi", "pods": "4", gpu: "2"}, zones=ZONES, capacity_types=("on-demand", "spot"))
    pods = _deployments(31, LABEL_ZONE) + _deployments(1, LABEL_ZONE, 40, 1, first=31)
    hosts = _deployments(31, LABEL_HOSTNAME, first=32) + _deployments(1, LABEL_HOSTNAME, 40, 2, first=63)
    if split:
        for i, p in enumerate(pods[-40:]):
            p.node_selector = {f"example.com/k{i % 2:02d}": "v"}
    for p in hosts:
        p.uid = "h" + p.uid
    pods += hosts
    for i in range(150):
        sel = {f"example.com/k{i % custom_keys:02d}": "v"} if custom_keys and i % 3 == 0 else {}
        pods.append(_pod(f"z-plain-{i:05d}", "200m", "128Mi", node_selector=sel))
    for i, p in enumerate(pods):
        if i % 10 == 0:
            p.containers[0].requests[gpu] = "1"
    random.Random(seed).shuffle(pods)
    prov = fake.provisioner("default", len(its), labels={f"example.com/k{i:02d}": "v" for i in range(custom_keys)})
    return _problem(its, pods, nodes, provisioners=[prov])


CASES = {}


def _family(family, maker, rungs, name=None):
    for rung, want in rungs:
        CASES[(name or family) + f"_{rung}"] = (lambda rung=rung: maker(rung), want, family, rung)


_family("count", count_field, [(1022, TAKEN), (1023, TAKEN), (1024, (1, 2)), (1025, (1, 2))])
_family("count_existing", count_field_existing, [(1100, TAKEN), (1200, TAKEN)])
_family("existing", lambda e: LC.existing_nodes(replicas=100, existing=e, free=3), [(63, TAKEN), (64, TAKEN), (65, (1, 1))])
_family("exact_filter", exact_filter, [(7, TAKEN), (8, TAKEN), (9, (1, 3)), (10, (1, 3))])
CASES["exact_filter_8_then_fits"] = (lambda: exact_filter(8, wide=4, wide_memory="20Gi"), TAKEN, "exact_filter_fits", 8)
_family("nrc_selectors", nrc_selectors, [(50, TAKEN), (62, TAKEN), (63, TAKEN), (64, (1, 5)), (66, (1, 5))])
_family("nrc_children", nrc_children, [(12, TAKEN), (15, TAKEN), (16, (1, 5)), (21, (1, 5))])
_family("zonal", zonal_groups, [(63, TAKEN), (64, TAKEN), (65, (0, 0))])
CASES["zonal_crowd_64"] = (zonal_crowd, TAKEN, "zonal_crowd", 64)
_family("hostname", hostname_groups, [(31, TAKEN), (32, TAKEN), (33, (1, 1))])
# (the rung of a hostname case is GH: a spread counts once, a herd twice)
for g, a, want in ((0, 16, TAKEN), (0, 17, (1, 1)), (30, 1, TAKEN), (28, 2, TAKEN), (31, 1, (1, 1))):
    CASES[f"hostname_{g}_herds_{a}"] = (lambda g=g, a=a: hostname_groups(g, a), want, "hostname", g + 2 * a)
_family("keys", keys, [(13, TAKEN), (14, (1, 1)), (24, (1, 1))])
_family("type_words", type_words, [(8192, TAKEN), (8193, (1, 1))])
_family("ladders", ladders, [(600, TAKEN), (1400, TAKEN), (1900, (1, 1))])
_family("hostname_records", lambda n: records(n, LABEL_HOSTNAME), [(11, TAKEN), (12, TAKEN), (13, (1, 7))])
_family("zone_records", lambda n: records(n, LABEL_ZONE), [(7, TAKEN), (8, TAKEN), (9, (1, 7))])
_family("hostname_items", hostname_items, [(2, TAKEN), (3, TAKEN)])
_family("hostname_skew", hostname_skew, [(250, TAKEN), (251, (1, 7))])
for e, n in ((64, 384), (64, 385), (0, 449)):
    CASES[f"slots_{e}_{n}"] = (lambda e=e, n=n: one_pod_machines(e, n), TAKEN, "slots", e + n)
_family("node_count", node_count, [(3584, TAKEN), (3585, (1, 4))])
_family("templates", templates, [(8, TAKEN), (9, TAKEN), (10, TAKEN)])
CASES["combined_64"] = (combined, TAKEN, "combined", 64)
CASES["combined_65_a_deployment_split_by_its_selectors"] = (lambda: combined(split=True), (0, 0), "combined", 65)

UNSUPPORTED = lambda: hostname_items(4)      # noqa: E731  (refused by the flattening, not by a kernel)
GOLDEN = ["node_count_3584", "node_count_3585"]      # the oracle needs minutes for these: tests/golden/rr_limit_hashes.json (make_rr_limit_hashes.py)
TAKEN_ONLY = {"count_existing", "exact_filter_fits", "zonal_crowd", "hostname_items", "slots", "templates"}      # families that pin what must NOT trip a limit
FAMILIES = sorted({c[2] for c in CASES.values()})


def fingerprints(res):
    return {"fp": hashlib.sha256(json.dumps(res.canonical(), sort_keys=True).encode()).hexdigest(),
            "reasons": hashlib.sha256(json.dumps(sorted((int(k), int(v)) for k, v in res.reasons.items())).encode()).hexdigest()}


def one_pod_each(res, n):
    """The closed form of the node-count cases: n new nodes, node i holding queue entry i (identical pods: the queue keeps their order) and nothing else."""
    return [list(x.pods) for x in res.new_nodes] == [[i] for i in range(n)] and not res.unscheduled and not any(res.existing.values())


# ---- that a case stands where it says it does: read from the ORACLE's result (and the flat problem's dimensions) alone, one check per family ----
def _sizes(res):
    return sorted((len(n.pods) for n in res.new_nodes), reverse=True)


def _records(res):
    return {json.dumps({k: (r.complement, sorted(r.values)) for k, r in sorted(n.requirements.items())}) for n in res.new_nodes}


def _holding(p, res, prefix):
    """The new nodes that hold a pod whose uid starts with `prefix`, with how many such pods."""
    return [(n, k) for n, k in ((n, sum(1 for i in n.pods if p.pods[i].uid.startswith(prefix))) for n in res.new_nodes) if k]


def _exact_filter_stands(rung, p, res, dims):
    """The wide pod sits on a mem-box machine without a 15-cpu pod (every machine that has one refused it), and `rung` machines hold a 15-cpu pod each."""
    wide, cpu = _holding(p, res, "b-wide-"), _holding(p, res, "a-cpu-")
    return len(wide) == 1 and wide[0][0].instance_types == ["mem-box"] and all(n is not wide[0][0] for n, _ in cpu) and [k for _, k in cpu] == [1] * rung


STANDS = {
    "count": lambda rung, p, res, dims: _sizes(res)[0] == rung and not res.unscheduled,                       # one machine is filled to the last slot of its capacity
    "count_existing": lambda rung, p, res, dims: [len(v) for v in res.existing.values()] == [1100],
    "existing": lambda rung, p, res, dims: dims["E"] == rung and sum(1 for v in res.existing.values() if v) == rung,
    "exact_filter": _exact_filter_stands,
    "exact_filter_fits": lambda rung, p, res, dims: max(k for _, k in _holding(p, res, "b-wide-")) >= 2 and [k for _, k in _holding(p, res, "a-cpu-")] == [1] * rung,
    "nrc_selectors": lambda rung, p, res, dims: len(_records(res)) == rung,
    "nrc_children": lambda rung, p, res, dims: len({(n.requirements[TEAM].values, n.requirements[LABEL_ZONE].values) for n in res.new_nodes if len(n.requirements[LABEL_ZONE].values) == 1}) == 3 * rung,
    "zonal": lambda rung, p, res, dims: dims["G"] == rung and dims["GH"] == 0,
    "zonal_crowd": lambda rung, p, res, dims: dims["G"] == rung and not res.unscheduled,
    "hostname": lambda rung, p, res, dims: dims["GH"] == rung and dims["G"] == rung,
    "keys": lambda rung, p, res, dims: dims["K"] - KEYS_WITHOUT_LABELS == rung and not res.unscheduled,
    "type_words": lambda rung, p, res, dims: dims["T"] == rung and (dims["T"] + 63) // 64 == (128 if rung == 8192 else 129),
    "ladders": lambda rung, p, res, dims: dims["T"] == rung and len({it.capacity["cpu"] for it in p.instance_types}) == rung and dims["R"] == 3,
    "hostname_records": lambda rung, p, res, dims: dims["GH"] == rung and not res.unscheduled,
    "zone_records": lambda rung, p, res, dims: dims["G"] == rung and dims["GH"] == 0 and not res.unscheduled,
    "hostname_items": lambda rung, p, res, dims: dims["GH"] == rung and not res.unscheduled,
    "hostname_skew": lambda rung, p, res, dims: _sizes(res) == [40],                                          # (a skew that wide never binds: one machine)
    "slots": lambda rung, p, res, dims: len(p.nodes) + len(res.new_nodes) == rung and rung >= 448,            # node index 448 (existing nodes first) is there or is the next
    "templates": lambda rung, p, res, dims: dims["M"] == rung and len(res.unscheduled) == 8 and all(res.reasons.get(i, 0) for i in res.unscheduled),
    "combined": lambda rung, p, res, dims: (dims["G"], dims["GH"], dims["E"], dims["R"], dims["K"]) == (rung, 32, 64, 4, 16) and not res.unscheduled,
}
KEYS_WITHOUT_LABELS = 3      # K of a problem whose provisioner has no custom label (set from what the flattening reports: see `keys`)


def boundary_ok(family, taken_by_rung):
    """taken_by_rung: [(rung, taken)] of one family.  The taken rungs are a prefix in rung order; both sides are there (families of TAKEN_ONLY: the taken side only)."""
    flags = [t for _, t in sorted(taken_by_rung, key=lambda rt: (rt[0], rt[1]))]      # (one rung both taken and given back: not a prefix)
    prefix = flags == sorted(flags, reverse=True)
    return prefix and flags[0] and (family in TAKEN_ONLY or not flags[-1])
