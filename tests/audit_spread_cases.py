"""What tests/test_audit_spread.py (on the lane-fibre emulator) and tests/test_audit_spread_gpu.py (on the device) share: the comparison of the audit's third pass
with its reference (tests/audit_spread_ref.py, through tests/audit_harness.py), the hand-made problems -- zonal spreads on labelled existing nodes, where the rule is exact and the placement is
known from how the problem was made --, the tamper matrix and the shapes at which the kernels take another path.  Every function takes the scheduler module `S` it
is to go through (the HIP libraries' or the emulator's)."""
import copy

import numpy as np

import audit_harness as H
import audit_spread_ref as SR
import audit_topo_cases as TC
import test_fuzz as F
import test_fuzz_mid as T
import test_problem_arrays as PA
from karpenter_core_amd import fake
from karpenter_core_amd import workloads as W
from karpenter_core_amd.model import DO_NOT_SCHEDULE, LABEL_ZONE, Expr, Problem, TopologySpreadConstraint

B = SR.BITS
D = H.PASSES["spread"]      # the pass, and its comparison with the reference (tests/audit_harness.py)
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary
ZONES = (TC.Z1, TC.Z2, TC.Z3)
CHUNK = 256      # csrc/ks_audit_spread.inc KS_AS_CHUNK: commit numbers per chunk; a tile is 64


def sliced_batch_says_the_same(S, flats, whole):
    """The batch form walks its problems in slices of bounded scratch (64 MiB of chunk table, which no test's batch reaches): with the budget set to one problem a
    slice (KS_AUDIT_SPREAD_SLICE_WORDS, a diagnostic switch) the batch says what it said in one slice."""
    import os
    os.environ["KS_AUDIT_SPREAD_SLICE_WORDS"] = "1"
    try:
        sliced = S.audit_spread_batch(flats)
    finally:
        del os.environ["KS_AUDIT_SPREAD_SLICE_WORDS"]
    assert len(sliced) == len(whole) > 1
    for a, b in zip(sliced, whole):
        assert np.array_equal(a["pod_flags"], b["pod_flags"]) and summary(a) == summary(b), (summary(a), summary(b))
    return True


# ---------------------------------------------------------------------------------------------------------------- hand-made problems
def _spread(key, app, skew=1):
    return TopologySpreadConstraint(skew, key, DO_NOT_SCHEDULE, TC._sel(app))


def zonal(pods: int, per_zone: int = 2, plain: int = 0) -> Problem:
    """3 * per_zone roomy existing nodes, node i in zone i // per_zone, and `pods` tiny pods under one self-selecting spread over the zone with maxSkew 1 (plus `plain`
    pods under nothing).  Every recorder sits on a labelled existing node: the rule is exact.  The reference fills the zones in turn."""
    its = fake.instance_types(4)
    nodes = [TC._roomy("e%d" % i, ZONES[i // per_zone]) for i in range(3 * per_zone)]
    ps = [TC._pod("sp-%04d" % i, app="sp", cpu="1m", mem="1Mi", spread=[_spread(LABEL_ZONE, "sp")]) for i in range(pods)] + [TC._pod("zz-plain-%d" % i, cpu="1m", mem="1Mi") for i in range(plain)]
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=ps, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def zone_of(node: int, per_zone: int = 2) -> int:
    return node // per_zone


def in_commit_order(res, seq, pods):
    return sorted((int(p) for p in pods if res["pod_node"][p] >= 0), key=lambda p: int(seq[p]))


def racks_spread() -> Problem:
    """A topology key with 64 values: 64 existing nodes, node i in rack i, and three pods under a self-selecting spread over the rack with maxSkew 1: three racks."""
    its = fake.instance_types(4)
    nodes = [TC._roomy("n%02d" % i, TC.Z1, **{TC.RACK: "rack-%02d" % i}) for i in range(64)]
    pods = [TC._pod("rk-%d" % i, app="rk", spread=[_spread(TC.RACK, "rk")]) for i in range(3)]
    prov = fake.provisioner("open", len(its), requirements=[Expr(TC.RACK, "In", ["rack-%02d" % i for i in range(64)])])      # (the racks are domains because the provisioner names them)
    return Problem(instance_types=its, provisioners=[prov], pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def two_keys() -> Problem:
    """Six existing nodes -- zones 1 2 3 1 2 3, racks a b a b a b -- and four pods under two self-selecting spreads with maxSkew 1: over the zone, then over the rack.
    First fit: nodes 0, 1, 2, then (the rack a holds two, b one) node 1."""
    its = fake.instance_types(4)
    nodes = [TC._roomy("n%d" % i, ZONES[i % 3], **{TC.RACK: "rack-%s" % "ab"[i % 2]}) for i in range(6)]
    pods = [TC._pod("tk-%d" % i, app="tk", spread=[_spread(LABEL_ZONE, "tk"), _spread(TC.RACK, "tk")]) for i in range(4)]
    prov = fake.provisioner("open", len(its), requirements=[Expr(TC.RACK, "In", ["rack-a", "rack-b"])])
    return Problem(instance_types=its, provisioners=[prov], pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


# the problems whose genuine results the GPU tests of this pass audit -- and, with pods of their own added, those of the fourth and the sixth
GENUINE = {
    "mid (topology, limits)": lambda: T.mid_problem(0),
    "node filter": lambda: PA.build_case("filter"),
    "existing nodes": lambda: PA.build_case("r3"),
    "fuzz 0": lambda: F.fuzz_problem(0), "fuzz 3": lambda: F.fuzz_problem(3), "fuzz 5": lambda: F.fuzz_problem(5), "fuzz 11": lambda: F.fuzz_problem(11), "fuzz 16": lambda: F.fuzz_problem(16),
    "config3": lambda: W.config3(pods=140, sizes=3, seed=1),
    "config3, 700 pods": lambda: W.config3(pods=700, sizes=10, seed=7),
    "a zonal spread on labelled nodes": lambda: zonal(40, plain=3),
    "two keys": two_keys,
}


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix
TAMPER_NAMES = ["a pod moved to a fuller zone", "the same one commit earlier: the pod after it is pushed over too", "two commit numbers swapped: the skew holds at the end, not at the time",
                "two pods given one commit number"]
N_SPREAD, N_PLAIN = 6, 2


def tamper_problem() -> Problem:
    return zonal(N_SPREAD, plain=N_PLAIN)


def check_genuine(res, seq):
    """The genuine result fills zones 1, 2, 3, 1, 2, 3 in commit order; returns the spread pods in commit order and the two plain pods."""
    assert res["n_new"] == 0 and not len(res["unscheduled"])
    sp = in_commit_order(res, seq, range(N_SPREAD))
    assert [zone_of(int(res["pod_node"][p])) for p in sp] == [0, 1, 2, 0, 1, 2], [int(res["pod_node"][p]) for p in sp]
    return sp, [N_SPREAD, N_SPREAD + 1]


def tampers(res, seq):
    """[(name, edited copy of `res`, edited copy of `seq`, {pod: bits} -- every other pod must carry nothing)]"""
    sp, plain = check_genuine(res, seq)
    out = []

    def case(name):
        r, s = copy.deepcopy({k: v for k, v in res.items() if k != "key_value"}), np.array(seq, dtype=np.int32)
        want = {}
        out.append((name, r, s, want))
        return r, s, want
    r, s, want = case(TAMPER_NAMES[0])      # the sixth, at counts 2 2 1, into zone 1: 2 + 1 - 1 > 1
    r["pod_node"][sp[5]] = 0
    want[sp[5]] = B["SPREAD"]
    r, s, want = case(TAMPER_NAMES[1])      # the fifth, at 2 1 1, into zone 1: 3 > 1; the sixth then finds 3 1 1 and goes to zone 3: fine.  With the fourth (1 1 1 -> any) nothing
    r["pod_node"][sp[4]] = 0
    want[sp[4]] = B["SPREAD"]
    r["pod_node"][sp[5]] = 1                # ... and the sixth claimed into zone 1 as well: 3 + 1 - 1
    want[sp[5]] = B["SPREAD"]
    r, s, want = case(TAMPER_NAMES[2])      # the third (zone 3) and the fourth (zone 1) change places in time: zone 1 is chosen at 1 1 0
    s[sp[2]], s[sp[3]] = s[sp[3]], s[sp[2]]
    want[sp[3]] = B["SPREAD"]
    r, s, want = case(TAMPER_NAMES[3])
    s[plain[1]] = s[plain[0]]
    want[plain[0]] = want[plain[1]] = B["SEQ"]
    assert [o[0] for o in out] == TAMPER_NAMES
    return out


def _verdict(S, flat, claimed, s, want, n):
    want_f = np.zeros(n, dtype=np.uint32)
    for i, b in want.items():
        want_f[i] = b
    try:
        dev, flags = compare(S, flat, claimed, s)
    except AssertionError as e:
        return "device and reference differ: %s" % (e,)
    if dev["exact_pairs"] != dev["checked"]["SPREAD"]:
        return "labelled existing nodes only, and %d of %d pairs exact" % (dev["exact_pairs"], dev["checked"]["SPREAD"])
    return True if np.array_equal(dev["pod_flags"], want_f) else "flags %s, expected %s" % ({int(i): int(dev["pod_flags"][i]) for i in np.nonzero(dev["pod_flags"])[0]}, want)


def run_tamper_matrix(S):
    """Solve `tamper_problem`, audit the genuine result (clean, every pair exact) and every edit through the claimed form; returns [(name, True or what differs)]."""
    flat = S.FlatProblem(tamper_problem())
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    assert dev["checked"] == {"SEQ": N_SPREAD + N_PLAIN, "SPREAD": N_SPREAD} and dev["exact_pairs"] == N_SPREAD and dev["skipped_groups"] == 0, dev
    res, seq = flat.result_arrays(), flat.pod_seq()
    report = [(name, _verdict(S, flat, claimed, s, want, N_SPREAD + N_PLAIN)) for name, claimed, s, want in tampers(res, seq)]
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- shapes where the kernels take another path
SHAPE_NAMES = ["two chunk boundaries and a tile boundary", "a key of 64 values: the violation in value id 63", "two groups on two keys: the violation in the second",
               "P = 1", "G = 0 and n_new = 0", "no eligible group"]


def run_shapes(S):
    """[(name, True or what differs)] -- each shape solved (clean by device and reference) and, where it says so, one claimed edit."""
    report = []

    def shape(name, make, body):
        flat = S.FlatProblem(make())
        try:
            flat.solve(decode=False)
            dev = assert_clean(S, flat)
            ok = body(flat, dev)
        except AssertionError as e:
            ok = "%s" % (e,)
        flat.close()
        report.append((name, ok))

    def long_order(flat, dev):
        n = 2 * CHUNK + 65
        assert dev["checked"] == {"SEQ": n, "SPREAD": n} and dev["exact_pairs"] == n and dev["n_new"] == 0, dev
        res, seq = flat.result_arrays(), flat.pod_seq()
        res = {k: v for k, v in res.items() if k != "key_value"}
        sp = in_commit_order(res, seq, range(n))
        late = sp[n - 2]      # commit number 2 * CHUNK + 63: the last lane of the first tile of the third chunk.  n - 2 = 3 * 192 - 1: the counts are 192 192 191
        count = [sum(1 for p in sp[:n - 2] if zone_of(int(res["pod_node"][p])) == z) for z in range(3)]
        assert sorted(count) == [191, 192, 192] and int(seq[late]) == 2 * CHUNK + 63 and zone_of(int(res["pod_node"][late])) == count.index(191), (count, int(seq[late]))
        res["pod_node"][late] = 2 * count.index(192)
        dev, flags = compare(S, flat, res, seq)
        got = {int(i): int(flags[i]) for i in np.nonzero(flags)[0]}
        assert got.get(late) == B["SPREAD"] and set(got) <= {late, sp[n - 1]} and dev["exact_pairs"] == n, got
        return True
    shape(SHAPE_NAMES[0], lambda: zonal(2 * CHUNK + 65), long_order)

    def rack_63(flat, dev):
        res, seq, prob = flat.result_arrays(), flat.pod_seq(), SR.problem_arrays(S, flat)
        res = {k: v for k, v in res.items() if k != "key_value"}
        k = [i for i in range(prob["K"]) if int(prob["key_nvalues"][i]) == 64]
        assert len(k) == 1 and int(prob["en.mask"][63 * prob["K"] + k[0]]) == 1 << 63 and dev["checked"]["SPREAD"] == 3 and sorted(res["pod_node"]) == [0, 1, 2], (k, res["pod_node"])
        sp = in_commit_order(res, seq, range(3))
        res["pod_node"][sp[1]] = res["pod_node"][sp[2]] = 63      # two into the rack of value id 63: the later of them finds 1 + 1 - 0
        dev, flags = compare(S, flat, res, seq)
        assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == {sp[2]: B["SPREAD"]}, flags
        return True
    shape(SHAPE_NAMES[1], racks_spread, rack_63)

    def second_key(flat, dev):
        res, seq = flat.result_arrays(), flat.pod_seq()
        res = {k: v for k, v in res.items() if k != "key_value"}
        sp = in_commit_order(res, seq, range(4))
        assert [int(res["pod_node"][p]) for p in sp] == [0, 1, 2, 1] and dev["checked"]["SPREAD"] == 8 and dev["exact_pairs"] == 8, ([int(res["pod_node"][p]) for p in sp], dev["checked"])
        res["pod_node"][sp[3]] = 3      # node 3 is in zone 1 (at 1 1 1: fine) and in rack b, as node 1 is: still clean
        dev, flags = compare(S, flat, res, seq)
        assert not flags.any(), flags
        res["pod_node"][sp[3]] = 4      # zone 2 at 1 1 1: fine; rack a at 2 1: 2 + 1 - 1 > 1
        dev, flags = compare(S, flat, res, seq)
        assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == {sp[3]: B["SPREAD"]}, flags
        return True
    shape(SHAPE_NAMES[2], two_keys, second_key)
    shape(SHAPE_NAMES[3], lambda: TC.plain(1), lambda flat, dev: True if (dev["checked"], dev["n_new"], dev["skipped_groups"], dev["exact_pairs"]) == ({"SEQ": 1, "SPREAD": 0}, 1, 0, 0) else str(dev))
    shape(SHAPE_NAMES[4], lambda: TC.plain(3, True), lambda flat, dev: True if (dev["checked"], dev["n_new"], dev["skipped_groups"]) == ({"SEQ": 3, "SPREAD": 0}, 0, 0) and flat.dims["G"] == 0 else str(dev))
    # the second pass's tamper cluster: its only spread is over the hostname
    shape(SHAPE_NAMES[5], TC.tamper_problem, lambda flat, dev: True if dev["checked"]["SPREAD"] == 0 and dev["skipped_groups"] == 1 and dev["checked"]["SEQ"] == len(TC.PODS) else str(dev))
    assert [r[0] for r in report] == SHAPE_NAMES
    return report
