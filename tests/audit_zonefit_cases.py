"""What tests/test_audit_zonefit.py (on the lane-fibre emulator) and tests/test_audit_zonefit_gpu.py (on the device) share: the comparison of the audit's ninth pass with
its reference (tests/audit_zonefit_ref.py, through tests/audit_harness.py's Pass), the `zonal_cluster(seed)` family, a hand-made problem whose first fit is known from
how it was made, the tamper matrix, the claimed results with indices out of range and the shapes at which the kernels take another path.  Every function takes the
scheduler module `S` it is to go through (the HIP libraries' or the emulator's)."""
import os
import random

import numpy as np

import audit_cases as C
import audit_firstfit_cases as FC
import audit_harness as H
from audit_harness import _claimable, flagged
import audit_hostfit_cases as HC
import audit_topo_cases as TC
import audit_zonefit_ref as ZR
from karpenter_core_amd import fake
from karpenter_core_amd.model import DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_ZONE, Expr, PreferredTerm, Problem, Taint, Toleration, TopologySpreadConstraint

B = ZR.BITS
ZFIT = B["ZFIT_EXISTING"] | B["ZFIT_NEW"]
Z1, Z2, Z3 = C.Z1, C.Z2, C.Z3
ZONES = [Z1, Z2, Z3]
COUNTERS = ("admitting_pairs", "exact_pods", "skipped_pods", "mixed_pods", "eligible_groups", "skipped_groups", "n_new", "n_placed")


class _Pass(H.Pass):
    """tests/audit_harness.py's descriptor for a pass that file does not list"""

    def __init__(self):
        self.name, self.ref, self.pod_bits, self.node_bits, self.checked, self.ref_returns, self.gives = "zonefit", ZR, ZR.BITS, None, ZR.CHECKED, None, ("pod_flags",)
        self.counters, self.pods_identity, self.extra, self.seq = COUNTERS, True, None, True
        self.summary_of = (("admitting", "admitting_pairs"), ("exact", "exact_pods"), ("skipped", "skipped_pods"), ("mixed", "mixed_pods"), ("groups", ("eligible_groups", "skipped_groups")),
                           ("n_new", "n_new"), ("n_placed", "n_placed"))
        self.method = self.stem = "audit_zonefit"
        self.batch, self.out, self.tables = "audit_zonefit_batch", "_AuditZoneFitOut", ("pod",)


D = _Pass()
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary


def _zspread(skew, app, key=LABEL_ZONE):
    return TopologySpreadConstraint(skew, key, DO_NOT_SCHEDULE, TC._sel(app))


def _problem(pods, nodes=(), types=4, extra_types=(), provs=None):      # provs: the open provisioner's requirements
    its = fake.instance_types(types) + list(extra_types)
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its), requirements=provs)], pods=list(pods), nodes=list(nodes), extra_well_known=fake.EXTRA_WELL_KNOWN)


# ---------------------------------------------------------------------------------------------------------------- the family
def zonal_cluster(seed: int, scale: int = 1) -> Problem:
    """12 to 24 existing nodes labelled over three zones, several with room; pods under self-selecting zonal spread with maxSkew 1 and 2, some with a zone preference
    for two zones (so that `among` is narrower than the registered set); and zonal pods too large for any existing node, which open machines.  scale: every count times as many (tools/time_audit.py's `zonal` leg)."""
    rng = random.Random(seed)
    E = rng.randint(12, 24) * scale
    nodes = []
    for i in range(E):
        n = C._node("e%04d" % i if scale > 1 else "e%02d" % i, ZONES[i % 3] if i < 3 else rng.choice(ZONES), rng.choice(["200m", "700m", "2", "4"]))
        nodes.append(n)
    pods = []
    for a, (app, skew) in enumerate((("za", 1), ("zb", 2), ("zc", 1))):
        for i in range(rng.randint(8, 14) * scale):
            two = rng.sample(ZONES, 2)
            kw = {"preferred_affinity": [PreferredTerm(1, [Expr(LABEL_ZONE, "In", two)])]} if (app == "zc" and i % 2) else {}      # (a preference: the group keeps its empty node filter)
            pods.append(TC._pod("%s-%04d" % (app, i) if scale > 1 else "%s-%02d" % (app, i), app=app, cpu="%dm" % rng.choice([150, 300, 450]), spread=[_zspread(skew, app)], **kw))
    for i in range(rng.randint(4, 8) * scale):      # too large for an existing node (at most 4 cores): these open machines
        pods.append(TC._pod("big-%04d" % i if scale > 1 else "big-%02d" % i, app="big", cpu="%dm" % rng.choice([4500, 5000]), mem="1Gi", spread=[_zspread(rng.choice([1, 2]), "big")]))
    for i in range(4):
        pods.append(TC._pod("plain-%02d" % i, cpu="100m"))
    return _problem(pods, nodes, types=12)


SEEDS = [1, 2, 3, 4]      # chosen on the CPU: in every one the reference alone examines pods against both kinds of target, with admitting pairs and exact pods (test_audit_zonefit.py asserts it)


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix
TAMPER_NAMES = ["a zonal pod moved to a later existing node of the same zone", "a zonal pod moved to a later existing node of another zone that the skew allows",
                "the last zonal pod of a new node claimed as the opener of an added node", "a placed pod claimed unscheduled",
                "commit order A: the earlier node's zone was admissible at s, not under the final counts", "commit order B: the earlier node's zone is admissible under the final counts, not at s",
                "an earlier node without the zone label", "a class with a hostname group beside the zonal one"]
PODS = ["zn_0", "zn_1"] + ["za_%d" % i for i in range(5)] + ["zc_%d" % i for i in range(6)] + ["zb_%d" % i for i in range(4)] + ["mix"]
U0, E1, E2, E3, E4, E5, E6 = range(7)      # u0: no zone label and no room | e1 / e4: zone 1 | e2 / e5: zone 2 | e3 / e6: zone 3
N_EXISTING = 7


def tamper_problem() -> Problem:
    """Seven existing nodes -- u0 without the zone label and without room, then two roomy nodes per zone: e1 e4 | e2 e5 | e3 e6 -- and an open provisioner whose largest
    type holds 96 cores.  Every pod's requests differ, so the queue is the list below.  zn_0 / zn_1 (45 cores each, zonal spread maxSkew 2) open one
    machine together, in zone 1; za_0 .. za_4 (maxSkew 1) go to e1 e2 e3 e1 e2; zc_0 .. zc_5 (maxSkew 1) to e1 e2 e3 e1 e2 e3; zb_0 .. zb_3 (maxSkew 2) to e1 e1 e2 e2; `mix`
    owns a zonal and a hostname spread."""
    huge = fake.new_instance_type("huge", {"cpu": "96", "memory": "256Gi", "pods": "200"})
    u0 = TC._roomy("u0", Z1)
    del u0.labels[LABEL_ZONE]
    u0.available = {"cpu": "10m", "memory": "8Mi", "pods": "2000"}
    nodes = [u0] + [TC._roomy("e%d" % i, ZONES[(i - 1) % 3]) for i in range(1, 7)]
    pods = [TC._pod("zn_%d" % i, app="zn", cpu="%dm" % (45000 - i), spread=[_zspread(2, "zn")]) for i in range(2)]
    pods += [TC._pod("za_%d" % i, app="za", cpu="%dm" % (900 - 10 * i), spread=[_zspread(1, "za")]) for i in range(5)]
    pods += [TC._pod("zc_%d" % i, app="zc", cpu="%dm" % (700 - 10 * i), spread=[_zspread(1, "zc")]) for i in range(6)]
    pods += [TC._pod("zb_%d" % i, app="zb", cpu="%dm" % (500 - 10 * i), spread=[_zspread(2, "zb")]) for i in range(4)]
    pods += [TC._pod("mix", app="mix", cpu="50m", spread=[_zspread(1, "mix"), _zspread(1, "mix", LABEL_HOSTNAME)])]
    assert [p.uid for p in pods] == PODS
    return _problem(pods, nodes, types=6, extra_types=[huge])


def check_genuine(res, seq):
    pod = {n: i for i, n in enumerate(PODS)}
    where = {n: int(res["pod_node"][i]) for n, i in pod.items()}
    assert res["n_existing"] == N_EXISTING and res["n_new"] == 1 and not len(res["unscheduled"]), (res["n_existing"], res["n_new"], where)
    assert [where["za_%d" % i] for i in range(5)] == [E1, E2, E3, E1, E2] and [where["zc_%d" % i] for i in range(6)] == [E1, E2, E3, E1, E2, E3], where
    assert [where["zb_%d" % i] for i in range(4)] == [E1, E1, E2, E2] and where["zn_0"] == where["zn_1"] == N_EXISTING, where
    assert [int(seq[pod[n]]) for n in PODS] == list(range(len(PODS))), seq
    return pod


def tampers(prob, res, seq):
    """[(name, edited copy of `res`, edited copy of `seq`, {pod: bits} -- exactly these flags, on exactly these pods)]"""
    pod = check_genuine(res, seq)
    out = []

    def case(name):
        r, s, want = _claimable(res), np.array(seq, dtype=np.int32), {}
        out.append((name, r, s, want))
        return r, s, want
    r, s, want = case(TAMPER_NAMES[0])      # za_3 at counts (1, 1, 1): zone 1 admits, and e1 has room
    r["pod_node"][pod["za_3"]] = E4
    want[pod["za_3"]] = B["ZFIT_EXISTING"]
    r, s, want = case(TAMPER_NAMES[1])      # zb_3 at counts (2, 1, 0), maxSkew 2: zones 2 and 3 admit, so the third pass is content with e3 -- and e2 comes first
    r["pod_node"][pod["zb_3"]] = E3
    want[pod["zb_3"]] = B["ZFIT_EXISTING"]
    r, s, want = case(TAMPER_NAMES[2])      # the shape of the historical bug: the machine zn_1 joined, opened earlier and pinned to zone 3 by its opener, has room again
    HC.to_an_added_node(r, prob, pod["zn_1"], 0)
    want[pod["zn_1"]] = B["ZFIT_NEW"]
    r, s, want = case(TAMPER_NAMES[3])      # za_3 against the final state without it, counts (1, 2, 1): e1 / e4 and the machine (zone 1), e3 / e6 (zone 3) take it
    q = pod["za_3"]
    r["pod_node"][q] = -1
    s[s > s[q]] -= 1
    s[q] = -1
    r["unscheduled"] = np.array([q], dtype=np.int32)
    want[q] = ZFIT
    want[pod["za_4"]] = B["ZFIT_EXISTING"]      # (and without za_3 before it, za_4 met counts (1, 1, 1): e1 would have taken it)
    r, s, want = case(TAMPER_NAMES[4])      # za_1, on e2, claimed to have committed before za_0: at counts (0, 0, 0) zone 1 admitted and e1 had room.  Under the final counts (2, 2, 1) zone 1 does not admit
    s[pod["za_0"]], s[pod["za_1"]] = s[pod["za_1"]], s[pod["za_0"]]
    want[pod["za_1"]] = B["ZFIT_EXISTING"]
    r, s, want = case(TAMPER_NAMES[5])      # zc_1, on e2 as it is: at counts (1, 0, 0) zone 1 refused it, though under the final counts (2, 2, 2) it admits.  zc_4's and zc_5's numbers change hands: no earlier node gains a zone
    s[pod["zc_4"]], s[pod["zc_5"]] = s[pod["zc_5"]], s[pod["zc_4"]]
    r["pod_node"][pod["zc_4"]], r["pod_node"][pod["zc_5"]] = E3, E2
    r, s, want = case(TAMPER_NAMES[6])      # u0 comes before every node and carries no zone label: it is no target, whatever it holds.  (za_0 moved from e1 to e4 is flagged for e1 alone)
    r["pod_node"][pod["za_0"]] = E4
    want[pod["za_0"]] = B["ZFIT_EXISTING"]
    r, s, want = case(TAMPER_NAMES[7])      # `mix` moved to a later node of its zone: not this pass's pod
    r["pod_node"][pod["mix"]] = int(res["pod_node"][pod["mix"]]) + 3
    assert [o[0] for o in out] == TAMPER_NAMES
    return out


def run_tamper_matrix(S):
    """Solve `tamper_problem`, audit the genuine result (clean) and every edit through the claimed form; every edit leaves the first pass clean, and every flagged one is
    silent under the fourth and the sixth pass; returns [(name, True or what differs)]."""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    n = len(PODS)
    assert dev["checked"]["PODS"] == n - 1 and dev["skipped_pods"] == 1 and dev["mixed_pods"] == 1 and dev["admitting_pairs"] > 0 and dev["exact_pods"] == n - 1, dev
    assert dev["checked"]["ZONE"] > dev["checked"]["STATIC"] > 0, dev      # (u0 fails the zone test for every pod)
    prob, res, seq = ZR.problem_arrays(S, flat), flat.result_arrays(), flat.pod_seq()
    report = []
    for name, claimed, s, want in tampers(prob, res, seq):
        try:
            d, flags = compare(S, flat, claimed, s)
            ok = True if flagged(d["pod_flags"]) == want else "flags %s, expected %s" % (flagged(d["pod_flags"]), want)
        except AssertionError as e:
            ok = "device and reference differ: %s" % (e,)
        if ok is True:
            first = flat.audit(claimed)
            if first["n_pods_flagged"] or first["n_nodes_flagged"]:
                ok = "the first pass flags the edit: %s %s" % (first["pod_bit_count"], first["node_bit_count"])
        if ok is True and want:
            for other in (flat.audit_firstfit(claimed, s), flat.audit_hostfit(claimed, s)):
                if other["n_pods_flagged"]:
                    ok = "another first-fit pass flags the edit: %s" % (other["pod_bit_count"],)
        if ok is True and name == TAMPER_NAMES[1] and flat.audit_spread(claimed, s)["n_pods_flagged"]:
            ok = "the third pass flags the edit"
        if ok is True and name == TAMPER_NAMES[7] and d["mixed_pods"] != 1:
            ok = "mixed_pods %d" % d["mixed_pods"]
        report.append((name, ok))
    flat.close()
    return report


def refusal_totals(out, flat):
    """what the pass's own counters must say when no table is given (tests/audit_harness.py `refusals`)"""
    return out.eligible_groups + out.skipped_groups == flat.dims["G"] and out.checked[1] + out.skipped_pods == flat.dims["P"] and out.checked[1] == len(PODS) - 1 and out.mixed_pods == 1


# ---------------------------------------------------------------------------------------------------------------- claimed results with indices out of range
RANGE_NAMES = ["pod_node far out of range", "pod_node == E + n_new", "pod_stage out of range", "node_tmpl out of range", "pod_seq out of range", "every index out of range at once"]


def run_range_cases(S):
    """Out-of-range pod_node, pod_stage, node_tmpl and pod_seq in a claimed result of `tamper_problem`: device and reference agree -- flags or skips.  (An index that
    addressed memory past a table would not agree with a reference that never reads it.)"""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    res, seq = flat.result_arrays(), flat.pod_seq()
    pod = check_genuine(res, seq)
    big, small = 2 ** 31 - 1, -2 ** 31

    def edit(name, r, s):
        if name == RANGE_NAMES[0]:
            r["pod_node"][pod["za_0"]], r["pod_node"][pod["zc_1"]], r["pod_node"][pod["zn_0"]] = big, small, -7
        elif name == RANGE_NAMES[1]:
            r["pod_node"][pod["za_1"]] = N_EXISTING + int(r["n_new"])
        elif name == RANGE_NAMES[2]:
            r["pod_stage"][pod["za_0"]], r["pod_stage"][pod["zb_1"]], r["pod_stage"][pod["zn_1"]] = big, small, 1
        elif name == RANGE_NAMES[3]:
            r["node_tmpl"][0] = big
        elif name == RANGE_NAMES[4]:
            s[pod["za_0"]], s[pod["zc_0"]], s[pod["zn_0"]], s[pod["zb_0"]] = big, small, len(PODS), -1
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
RACK = "example.com/rack"


def _racked(name, zone, rack, room=True, **labels):
    n = TC._roomy(name, zone, **dict({RACK: rack}, **labels))
    if not room:
        n.available = {"cpu": "10m", "memory": "8Mi", "pods": "2000"}
    return n


def _open_over(**values):
    """the open provisioner's requirements `key In values`, one per custom key: the values are the key's registered domains (a node's label alone registers none)"""
    return [Expr(k, "In", list(v)) for k, v in values.items()]


def round_robin(n: int) -> Problem:
    """n pods of falling size under one self-selecting zonal spread with maxSkew 1 over e0 / e1 / e2 (zones 1 / 2 / 3) and three later nodes e3 / e4 / e5: the pod with
    commit number s goes to e(s mod 3), and which zones admit it is a matter of the prefix at s to the unit."""
    nodes = [TC._roomy("e%d" % i, ZONES[i % 3]) for i in range(6)]
    for x in nodes:
        x.available = {"cpu": "4000", "memory": "64Gi", "pods": "5000"}
    return _problem([TC._pod("r%04d" % i, app="r", cpu="%dm" % (2000 - i), mem="1Mi", spread=[_zspread(1, "r")]) for i in range(n)], nodes)


def last_value(n: int = 64) -> Problem:
    """n existing nodes, node i alone in rack i; n pods under one self-selecting spread over the rack with maxSkew 1: pod i fills rack i, and the last pod is admitted
    by the last value of the key alone."""
    return _problem([TC._pod("v%02d" % i, app="v", cpu="%dm" % (900 - i), spread=[_zspread(1, "v", RACK)]) for i in range(n)], [_racked("e%02d" % i, ZONES[i % 3], "r%02d" % i) for i in range(n)],
                    provs=_open_over(**{RACK: ["r%02d" % i for i in range(n)]}))


def two_keys() -> Problem:
    """e0 (zone 1, rack a) and e1 (zone 2, rack b); t_0 and t_1 own a zonal spread with maxSkew 5 and a rack spread with maxSkew 1, both self-selecting: the zone would let
    t_1 join t_0 on e0, the rack -- the class's second group -- refuses."""
    sp = lambda: [_zspread(5, "t"), _zspread(1, "t", RACK)]
    return _problem([TC._pod("t_%d" % i, app="t", cpu="%dm" % (500 - i), spread=sp()) for i in range(2)], [_racked("e0", Z1, "a"), _racked("e1", Z2, "b")], provs=_open_over(**{RACK: "ab"}))


KEYS5 = [LABEL_ZONE, RACK, "example.com/row", "example.com/room", "example.com/site"]


def many_groups() -> Problem:
    """`four` owns spreads over four keys (KS_AZ_GROUPS: examined), `five` over five (skipped); two nodes that carry every key."""
    lab = lambda i: {k: "v%d" % i for k in KEYS5[2:]}
    nodes = [_racked("e0", Z1, "a", **lab(0)), _racked("e1", Z2, "b", **lab(1))]
    pods = [TC._pod("five", app="five", cpu="300m", spread=[_zspread(1, "five", k) for k in KEYS5]), TC._pod("four", app="four", cpu="200m", spread=[_zspread(1, "four", k) for k in KEYS5[:4]])]
    return _problem(pods, nodes, provs=_open_over(**dict({RACK: "ab"}, **{k: ["v0", "v1"] for k in KEYS5[2:]})))


def one_node_admits(E: int, at: int) -> Problem:
    """E existing nodes in zone 1 of which only `at` and the last have room, and one pod under a self-selecting zonal spread: it goes to `at`."""
    return _problem([TC._pod("s", app="s", cpu="500m", spread=[_zspread(1, "s")])], [_racked("e%03d" % i, Z1, "a", room=i in (at, E - 1)) for i in range(E)])


def one_type_fits(T: int = 65) -> Problem:
    """The ladder of T types -- type i has i + 1 cores -- and two pods of 32 cores under one self-selecting zonal spread with maxSkew 2: they share a machine that only
    the largest type makes."""
    return _problem([TC._pod("w_%d" % i, app="w", cpu="%dm" % (32000 - i), mem="64Mi", spread=[_zspread(2, "w")]) for i in range(2)], types=T)


def plain_only() -> Problem:
    return _problem([TC._pod("p%d" % i, cpu="%dm" % (100 + i)) for i in range(5)], [TC._roomy("e0", Z1)])


NODE_SHAPES = [(65, 0), (65, 63), (257, 0), (257, 255)]
SHAPE_NAMES = ["2 x 256 + 65 pods: the offender just behind a tile and a chunk boundary", "a key of 64 values: the only admissible one is the last", "two groups on two keys: the second refuses",
               "a class at KS_AZ_GROUPS groups, and one above it", "E = 0", "n_new = 0", "P = 1", "no eligible group"] + \
              ["E = %d: the only admitting node at index %d" % ns for ns in NODE_SHAPES] + ["T = 65: the only admitting type in the last bit", "three runs, the same bytes",
                                                                                          "one problem per slice"]


def run_shapes(S):
    """[(name, True or what differs)] -- each shape solved (clean by device and reference) and, where it says so, claimed edits."""
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
            ok = "%s: %s" % (type(e).__name__, str(e)[:500])
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

    def boundaries(flat, dev):
        n = 2 * 256 + 65
        res, seq = flat.result_arrays(), flat.pod_seq()
        assert flat.dims["P"] == n and [int(x) for x in seq] == list(range(n)) and [int(x) for x in res["pod_node"]] == [i % 3 for i in range(n)], (seq[:8], res["pod_node"][:8])
        assert dev["checked"]["PODS"] == n and dev["exact_pods"] == n, dev
        for sq in (64, 65, 256, 257, 512, n - 1):      # moved to the later node of its zone: the node it left comes first; the zones before it in the round refused it at s
            got = claim(flat, move(sq, sq % 3 + 3))
            assert got == {sq: B["ZFIT_EXISTING"]}, (sq, got)
        return True
    shape(SHAPE_NAMES[0], lambda: round_robin(2 * 256 + 65), boundaries)

    def last(flat, dev):
        res = flat.result_arrays()
        assert [int(x) for x in res["pod_node"]] == list(range(64)) and dev["eligible_groups"] == 1 and dev["checked"]["PODS"] == 64, (res["pod_node"], dev)
        prob = ZR.problem_arrays(S, flat)
        g = [i for i in range(prob["G"]) if int(prob["grp_type"][i]) == 0][0]
        k = int(prob["grp_key"][g])
        assert int(prob["key_nvalues"][k]) == 64 and (int(prob["en.mask"][63 * prob["K"] + k]) >> 63) & 1, (prob["key_nvalues"][k], prob["en.mask"][63 * prob["K"] + k])
        got = claim(flat, unschedule(63))      # every other rack holds a pod: value 63 alone admits
        assert got == {63: B["ZFIT_EXISTING"]}, got
        return True
    shape(SHAPE_NAMES[1], last_value, last)
    shape(SHAPE_NAMES[2], two_keys, lambda flat, dev: True if [int(x) for x in flat.result_arrays()["pod_node"]] == [0, 1] and dev["eligible_groups"] == 2 and dev["checked"]["PODS"] == 2 and
          dev["checked"]["ZONE"] == 4 and dev["checked"]["STATIC"] == 3 else str(dev))      # (t_0: both nodes pass; t_1: e0 fails on the rack)
    shape(SHAPE_NAMES[3], many_groups, lambda flat, dev: True if int(flat.result_arrays()["pod_node"].min()) >= 0 and dev["eligible_groups"] == 9 and dev["checked"]["PODS"] == 1 and dev["skipped_pods"] == 1 and dev["mixed_pods"] == 0 else str(dev))
    shape("E = 0", one_type_fits, lambda flat, dev: True if flat.dims["E"] == 0 and dev["n_new"] == 1 and dev["checked"]["PODS"] == 2 and dev["checked"]["ZONE"] == 0 else str(dev))
    shape("n_new = 0", lambda: round_robin(3), lambda flat, dev: True if dev["n_new"] == 0 and dev["checked"]["PODS"] == 3 and dev["checked"]["ZONE"] == 18 else str(dev))
    shape("P = 1", lambda: one_node_admits(2, 0), lambda flat, dev: True if flat.dims["P"] == 1 and dev["checked"] == {"SEQ": 1, "PODS": 1, "ZONE": 2, "STATIC": 2} and dev["admitting_pairs"] == 2 else str(dev))
    shape("no eligible group", plain_only, lambda flat, dev: True if dev["eligible_groups"] == 0 and dev["checked"] == {"SEQ": 5, "PODS": 0, "ZONE": 0, "STATIC": 0} and dev["skipped_pods"] == 5 else str(dev))

    def only_node(E, at):
        def body(flat, dev):
            assert flat.dims["E"] == E and int(flat.result_arrays()["pod_node"][0]) == at and dev["checked"] == {"SEQ": 1, "PODS": 1, "ZONE": E, "STATIC": E} and dev["admitting_pairs"] == 2, dev
            got = claim(flat, move(0, E - 1))      # the minimum over the existing nodes crosses lanes, waves and workgroups
            assert got == {0: B["ZFIT_EXISTING"]}, got
            return True
        return body
    for (E, at), name in zip(NODE_SHAPES, SHAPE_NAMES[8:12]):
        shape(name, lambda E=E, at=at: one_node_admits(E, at), only_node(E, at))

    def last_type(flat, dev):
        prob, res = ZR.problem_arrays(S, flat), flat.result_arrays()
        words = np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, 2)
        assert flat.dims["T"] == 65 and res["n_new"] == 1 and [int(w) for w in words[0]] == [0, 1] and [int(x) for x in res["pod_node"]] == [0, 0], (words, res["pod_node"])

        def edit(r, s):
            HC.to_an_added_node(r, prob, 1, 0)
        got = claim(flat, edit)      # the machine w_1 joined has room again: the walk over the types must reach the one bit to say so
        assert got == {1: B["ZFIT_NEW"]}, got
        return True
    shape(SHAPE_NAMES[12], one_type_fits, last_type)

    def same_bytes():
        def claimed(f):
            r, s = _claimable(f.result_arrays()), np.array(f.pod_seq(), dtype=np.int32)
            r["pod_node"][PODS.index("za_3")] = E4
            return r, s
        first = H.same_flags_every_run(D, S, tamper_problem(), claimed)
        return True if flagged(first["pod_flags"]) == {PODS.index("za_3"): B["ZFIT_EXISTING"]} else str(flagged(first["pod_flags"]))
    try:
        ok = same_bytes()
    except Exception as e:
        ok = "%s: %s" % (type(e).__name__, str(e)[:500])
    report.append((SHAPE_NAMES[13], ok))

    def slices():
        flats = [S.FlatProblem(p) for p in (tamper_problem(), round_robin(70), two_keys())]
        S.solve_batch(flats, decode=False)
        whole = S.audit_zonefit_batch(flats)
        os.environ["KS_AUDIT_SPREAD_SLICE_WORDS"] = "1"      # the third pass's diagnostic switch: one problem per slice
        try:
            sliced = S.audit_zonefit_batch(flats)
        finally:
            del os.environ["KS_AUDIT_SPREAD_SLICE_WORDS"]
        ones = [assert_clean(S, f) for f in flats]
        for f in flats:
            f.close()
        return True if all(np.array_equal(a["pod_flags"], b["pod_flags"]) and np.array_equal(a["pod_flags"], c["pod_flags"]) and summary(a) == summary(b) == summary(c) and a["checked"]["PODS"] > 0
                           for a, b, c in zip(whole, sliced, ones)) else str([(summary(a), summary(b)) for a, b in zip(whole, sliced)])
    try:
        ok = slices()
    except Exception as e:
        ok = "%s: %s" % (type(e).__name__, str(e)[:500])
    report.append((SHAPE_NAMES[14], ok))
    assert [r[0] for r in report] == SHAPE_NAMES, [r[0] for r in report]
    return report


# ---------------------------------------------------------------------------------------------------------------- two clauses of the new-node predicate, through this pass's kernels
# The class is under one zonal spread group, so it names no node selector of its own (the group keeps its empty node filter): the fillers pin their machine to zone 1
# and to the six-core type, and only the new-node path exists.
PINNED = {LABEL_ZONE: Z1}


def _zonal_taint_pair():
    """Two pods fill a machine of `open`, pinned to zone 1; `tolerant` and `intolerant`, each under a zonal spread of its own and too large in memory to share a machine, open the next two.  Claimed: the first
    machine has room to the milli-unit for the target and is of the second template, which taints its machines -- the target is `intolerant`, then `tolerant`."""
    its = fake.instance_types(6)
    provs = [fake.provisioner("open", len(its), weight=10), fake.provisioner("tainted", len(its), weight=1, taints=[Taint("dedicated", "x")])]
    pods = [FC.six_core_pod("first", "2500m", PINNED), FC.six_core_pod("second", "2500m", PINNED),
            TC._pod("tolerant", app="t", cpu="2400m", mem="7Gi", spread=[_zspread(1, "t")], tolerations=[Toleration(key="dedicated", operator="Exists")]),
            TC._pod("intolerant", app="i", cpu="2300m", mem="7Gi", spread=[_zspread(1, "i")])]
    make = lambda: FC.clause_problem(pods, provs)

    def edit(r, s, prob, admit):
        target = 2 if admit else 3
        j0, j1 = FC.opened_in_order(r, s, prob, 0, target)
        assert FC.new_node_of(prob, r, 1) == j0 and int(r["node_tmpl"][j0]) == 0 and int(prob["tmpl_taints"][1]) and not int(prob["tmpl_taints"][0]), (r["node_tmpl"], prob["tmpl_taints"])
        FC.boundary_requests(r, prob, j0, FC.class_of(prob, r, target), 0)
        r["node_tmpl"][j0] = 1
        return target
    return make, edit, "ZFIT_NEW"


CLAUSE_PAIRS = [FC.FITS_NAMES + (lambda: FC.fits_pair("ZFIT_NEW", PINNED, app="z", spread=[_zspread(1, "z")]),), FC.TAINT_NAMES + (_zonal_taint_pair,)]
CLAUSE_NAMES = FC.clause_names(CLAUSE_PAIRS)


def run_clauses(S):
    """tests/audit_firstfit_cases.py's Fits pair, and a taint pair, on classes under one zonal spread group: [(name, True or what differs)]"""
    return FC.run_clause_pairs(S, CLAUSE_PAIRS, compare, assert_clean, ZR.problem_arrays, B, B["ZFIT_NEW"])
