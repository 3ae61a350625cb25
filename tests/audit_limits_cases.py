"""What tests/test_audit_limits.py (on the lane-fibre emulator) and tests/test_audit_limits_gpu.py (on the device) share: the comparison of the audit's fifth pass
with its reference (tests/audit_limits_ref.py, through tests/audit_harness.py), the hand-made problems -- a provisioner `capped` with a cpu limit over the ladder of instance types, where the
reference's openings are known from how the problem was made --, the tamper matrix, the pinned one-sidedness and the shapes at which the kernels take another path.
Every function takes the scheduler module `S` it is to go through (the HIP libraries' or the emulator's)."""
import random

import numpy as np

import audit_cases as C
import audit_harness as H
from audit_harness import _claimable, flagged
import audit_limits_ref as LR
import audit_topo_cases as TC
from karpenter_core_amd import fake
from karpenter_core_amd.model import LABEL_PROVISIONER, Problem

PB, NB = LR.POD_BITS, LR.NODE_BITS
EXTRA, MISSING, LIMIT, SEQ = NB["LIMIT_EXTRA"], NB["LIMIT_MISSING"], PB["LIMIT_TEMPLATE"], PB["SEQ"]
D = H.PASSES["limits"]      # the pass, and its comparison with the reference (tests/audit_harness.py)
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary
KS_WHY_LIMITS = 1


def _type_words(res, j):
    return [int(w) for w in np.asarray(res["node_types"], dtype=np.uint64).reshape(int(res["n_new"]), -1)[j]]


def _set_types(res, j, bits):
    words = np.asarray(res["node_types"], dtype=np.uint64).reshape(int(res["n_new"]), -1).copy()
    for w in range(words.shape[1]):
        words[j, w] = np.uint64((bits >> (64 * w)) & ((1 << 64) - 1))
    res["node_types"] = words


def _types(res, j):
    return sum(w << (64 * i) for i, w in enumerate(_type_words(res, j)))


def _open_copy(r, s, j, pod):
    """`r` with one new node more -- a copy of new node j's rows, but the requests -- that unscheduled pod `pod` is claimed to have opened last"""
    n = int(r["n_new"])
    for name in ("node_tmpl", "node_types", "node_requests", "node_requests_present", "node_present", "node_complement", "node_mask", "node_gt", "node_lt", "node_it_state"):
        a = np.asarray(r[name]).reshape(n, -1)
        r[name] = np.concatenate([a, a[j:j + 1]]).reshape(-1) if name in ("node_tmpl", "node_requests_present", "node_present", "node_complement", "node_it_state") else np.concatenate([a, a[j:j + 1]])
    r["pod_node"][pod] = int(r["n_existing"]) + n
    s[pod] = int(s.max()) + 1
    r["unscheduled"] = np.array([u for u in r["unscheduled"] if u != pod], dtype=np.int32)
    r["n_new"] = n + 1


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix
def capped_problem(pods: int = 5, second: bool = True, types: int = 6, limit: str = "10") -> Problem:
    """The ladder of `types` instance types -- type i has i + 1 cores --, provisioner `capped` (weight 10, a cpu limit of 10) before `second` (weight 1, no limits) and
    pods of 2500m / 1Gi under no constraint.  With five pods: the first opens a six-core machine of `capped` (6 of 10 taken), the second joins it, the third opens a
    machine of `capped` out of the types within the remaining 4 cores -- fake-it-2, fake-it-3 --, the fourth and fifth go to `second`, or stay unscheduled."""
    its = fake.instance_types(types)
    provs = [fake.provisioner("capped", len(its), weight=10, limits={"cpu": limit})] + ([fake.provisioner("second", len(its), weight=1)] if second else [])
    return Problem(instance_types=its, provisioners=provs, pods=[TC._pod("p%d" % i, cpu="2500m", mem="1Gi") for i in range(pods)], nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def check_genuine(res, seq):
    assert res["n_new"] == 3 and not len(res["unscheduled"]), (res["n_new"], res["unscheduled"])
    assert [int(x) for x in res["pod_node"]] == [0, 0, 1, 2, 2] and [int(x) for x in res["node_tmpl"]] == [0, 0, 1], (res["pod_node"], res["node_tmpl"])
    assert [_types(res, j) for j in range(3)] == [0x20, 0x0C, 0x20], [hex(_types(res, j)) for j in range(3)]
    assert [int(s) for s in seq] == [0, 1, 2, 3, 4], seq


TAMPER_NAMES = ["node 1 given the five-core type", "node 1 reduced to one type", "node 2 billed to capped", "node 1 billed to second", "the commit numbers of nodes 0 and 1 exchanged",
                "capped alone: pod 2 claimed unscheduled", "the opener of node 1 shares a commit number, and node 2 is billed to capped"]


def run_tamper_matrix(S):
    """[(name, True or what differs)]: the genuine results are clean, each edit through the claimed form raises exactly the reference's flags and the bits expected."""
    report = []
    flat = S.FlatProblem(capped_problem(), flags=S.KS_FLAG_NO_RR)
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    assert dev["limited_templates"] == 1 and dev["exact_nodes"] == 2 and dev["binding_nodes"] >= 1 and dev["checked"]["NODES"] == 2 and dev["skipped_nodes"] == 0, dev
    res, seq = flat.result_arrays(), flat.pod_seq()
    check_genuine(res, seq)

    def verdict(name, f, edit, want_nodes, want_pods, more=None):
        try:
            r, s = _claimable(f.result_arrays()), np.array(f.pod_seq(), dtype=np.int32)
            edit(r, s)
            dev, ref = compare(S, f, r, s)
            got_n, got_p = flagged(dev["node_flags"]), flagged(dev["pod_flags"])
            ok = True
            if got_n != want_nodes or got_p != want_pods:
                ok = "nodes %s pods %s, expected %s %s" % (got_n, got_p, want_nodes, want_pods)
            if ok is True and more:
                ok = more(f, r, s, dev)
        except AssertionError as e:
            ok = "device and reference differ: %s" % (e,)
        report.append((name, ok))

    def others_silent(f, r, s, dev):
        first, fourth = f.audit(r), f.audit_firstfit(r, s)
        if first["n_pods_flagged"] or first["n_nodes_flagged"] or fourth["n_pods_flagged"]:
            return "another pass flags the edit: %s %s %s" % (first["pod_bit_count"], first["node_bit_count"], fourth["pod_bit_count"])
        return True

    def first_silent(f, r, s, dev):
        first = f.audit(r)
        return True if not first["n_nodes_flagged"] and not first["n_pods_flagged"] else "the first pass flags the edit: %s" % (first["node_bit_count"],)
    E = 0      # no existing node: new node j is node j
    verdict(TAMPER_NAMES[0], flat, lambda r, s: _set_types(r, 1, 0x0C | 0x10), {E + 1: EXTRA}, {}, others_silent)
    verdict(TAMPER_NAMES[1], flat, lambda r, s: _set_types(r, 1, 0x04), {E + 1: MISSING}, {}, first_silent)

    def bill2(r, s):
        r["node_tmpl"][2] = 0
    verdict(TAMPER_NAMES[2], flat, bill2, {E + 2: EXTRA}, {})      # U = 10 - 6 - 4 = 0

    def bill1(r, s):
        r["node_tmpl"][1] = 1
    verdict(TAMPER_NAMES[3], flat, bill1, {}, {2: LIMIT, 3: LIMIT})      # capped still had 4 cores at commit 2 -- and, with node 1 gone from its bill, at commit 3

    def exchange(r, s):
        s[:] = [1, 2, 0, 3, 4]
    verdict(TAMPER_NAMES[4], flat, exchange, {E + 1: MISSING}, {})      # L = 10 admits the five- and six-core types
    flat.close()

    alone = S.FlatProblem(capped_problem(pods=3, second=False), flags=S.KS_FLAG_NO_RR)
    alone.solve(decode=False)
    dev = assert_clean(S, alone)
    res = alone.result_arrays()
    assert res["n_new"] == 2 and [_types(res, j) for j in range(2)] == [0x20, 0x0C] and dev["exact_nodes"] == 2, (res["n_new"], dev)

    def unschedule(r, s):
        r["pod_node"][2], s[2], r["unscheduled"], r["n_new"] = -1, -1, np.array([2], dtype=np.int32), 1
        for name in ("node_tmpl", "node_requests_present", "node_present", "node_complement", "node_it_state"):
            r[name] = np.asarray(r[name])[:1].copy()
        for name in ("node_types", "node_requests", "node_mask", "node_gt", "node_lt"):
            r[name] = np.asarray(r[name]).reshape(2, -1)[:1].copy()
    verdict(TAMPER_NAMES[5], alone, unschedule, {}, {2: LIMIT})
    alone.close()

    flat = S.FlatProblem(capped_problem(), flags=S.KS_FLAG_NO_RR)
    flat.solve(decode=False)

    def collide(r, s):
        s[2] = s[3]
        r["node_tmpl"][2] = 0

    def skipped(f, r, s, dev):
        return True if dev["skipped_nodes"] == 1 and dev["exact_nodes"] == 0 else "skipped_nodes %d exact_nodes %d" % (dev["skipped_nodes"], dev["exact_nodes"])
    verdict(TAMPER_NAMES[6], flat, collide, {E + 2: EXTRA}, {2: SEQ, 3: SEQ}, skipped)      # node 1 is unordered: U_2 = 10 - 6 = 4 still refuses the six-core type
    flat.close()

    five = S.FlatProblem(capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR)      # with five pods, pods 3 and 4 are unscheduled for the limits
    five.solve(decode=False)
    try:
        dev = assert_clean(S, five)
        res = five.result_arrays()
        ok = True if [int(x) for x in res["unscheduled"]] == [3, 4] and [int(res["pod_reason"][p]) & 15 for p in (3, 4)] == [KS_WHY_LIMITS] * 2 else "unscheduled %s reasons %s" % (res["unscheduled"], res["pod_reason"])
    except AssertionError as e:
        ok = str(e)
    report.append(("capped alone, five pods: two unscheduled for the limits, clean", ok))
    five.close()
    assert [r[0] for r in report][:len(TAMPER_NAMES)] == TAMPER_NAMES
    return report


TAMPER_REPORT_NAMES = TAMPER_NAMES + ["capped alone, five pods: two unscheduled for the limits, clean"]


# ---------------------------------------------------------------------------------------------------------------- one-sidedness, pinned
ONE_SIDED_NAMES = ["genuine: U_1 = 7, L_1 = 2, node 1 not exact", "fake-it-4 added to node 1: between the bounds, not flagged", "fake-it-7 added to node 1: EXTRA", "fake-it-0 removed from node 1: MISSING"]


def one_sided_problem() -> Problem:
    """`capped` with cpu 10 over eight types; a (2500m) opens a machine of fake-it-2 .. 7, b (300m, integer == 3: fake-it-2 alone) joins it and narrows it to fake-it-2,
    c (200m) does not fit beside them and opens a machine.  What subtractMax took at a's opening was 8 cores, so 2 remained -- fake-it-0, fake-it-1 --; the final
    state says only that at least 3 were taken (U_1 = 7) and that a alone could have kept fake-it-7 (L_1 = 2)."""
    its = fake.instance_types(8)
    pods = [TC._pod("a", cpu="2500m", mem="1Gi"), TC._pod("b", cpu="300m", mem="64Mi", node_selector={fake.LABEL_INTEGER: "3"}), TC._pod("c", cpu="200m", mem="64Mi")]
    return Problem(instance_types=its, provisioners=[fake.provisioner("capped", len(its), weight=10, limits={"cpu": "10"})], pods=pods, nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def run_one_sided(S):
    report = []
    flat = S.FlatProblem(one_sided_problem(), flags=S.KS_FLAG_NO_RR)
    flat.solve(decode=False)
    try:
        dev = assert_clean(S, flat)
        res = flat.result_arrays()
        ok = True if res["n_new"] == 2 and [_types(res, j) for j in range(2)] == [0x04, 0x03] and [int(x) for x in res["pod_node"]] == [0, 0, 1] and dev["exact_nodes"] == 1 and dev["checked"]["NODES"] == 2 \
            else "types %s pods %s dev %s" % ([hex(_types(res, j)) for j in range(int(res["n_new"]))], res["pod_node"], dev)
    except AssertionError as e:
        ok = str(e)
    report.append((ONE_SIDED_NAMES[0], ok))
    for name, bits, want in zip(ONE_SIDED_NAMES[1:], (0x03 | 0x10, 0x03 | 0x80, 0x02), ({}, {1: EXTRA}, {1: MISSING})):
        try:
            r, s = _claimable(flat.result_arrays()), np.array(flat.pod_seq(), dtype=np.int32)
            _set_types(r, 1, bits)
            dev, ref = compare(S, flat, r, s)
            got = flagged(dev["node_flags"])
            ok = True if got == want and not dev["n_pods_flagged"] else "nodes %s pods %s, expected %s" % (got, flagged(dev["pod_flags"]), want)
        except AssertionError as e:
            ok = "device and reference differ: %s" % (e,)
        report.append((name, ok))
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- the seeded family
FAMILY_SEEDS = list(range(7000, 7044))
DEVICE_RESOURCE = "fake.com/vendor-a"


def family_problem(seed: int) -> Problem:
    """1 - 3 provisioners, at least one limited on one or two of cpu / memory / a device resource; 0 - 6 existing nodes of the limited provisioner, so that its
    remaining resources start low or negative; 10 - 60 pods under no constraint, a few of them asking for the device."""
    rng = random.Random(seed)
    nt = rng.choice([6, 8, 10, 12])
    its = fake.instance_types(nt)
    for i, it in enumerate(its):
        if i % 3 == 2:      # every third type carries devices
            its[i] = fake.new_instance_type(it.name, {"cpu": str(i + 1), "memory": "%dGi" % ((i + 1) * 2), "pods": str((i + 1) * 10), DEVICE_RESOURCE: str(1 + i // 3)})
    nprov = rng.randint(1, 3)
    lim_at = 0 if rng.random() < 0.7 else rng.randrange(nprov)      # (the limited provisioner is mostly the heaviest: its machines are the ones that open)
    existing = rng.randint(0, 6)
    provs = []
    for i in range(nprov):
        limits = None
        if i == lim_at or rng.random() < 0.3:
            names = rng.sample(["cpu", "memory", DEVICE_RESOURCE], rng.choice([1, 1, 2]))
            limits = {}
            for nm in names:
                limits[nm] = {"cpu": str(rng.randint(8, 48)), "memory": "%dGi" % rng.randint(16, 96), DEVICE_RESOURCE: str(rng.randint(2, 8))}[nm]
            if rng.random() < 0.08:
                limits = {}
        provs.append(fake.provisioner("prov%d" % i, len(its), weight=10 - i, limits=limits))
    nodes = []
    for e in range(existing):
        n = C._node("e%d" % e, C.Z1 if e % 2 else C.Z2, "%dm" % rng.choice([0, 100, 600]))
        n.labels[LABEL_PROVISIONER] = "prov%d" % lim_at
        cores = rng.choice([1, 2, 4])
        n.capacity = {"cpu": str(cores), "memory": "%dGi" % (2 * cores), "pods": "60"}
        nodes.append(n)
    pods = []
    for i in range(rng.randint(10, 60)):
        cpu = rng.choice(["200m", "500m", "900m", "1500m", "2500m", "3500m"])
        p = TC._pod("p%03d" % i, cpu=cpu, mem=rng.choice(["128Mi", "1Gi", "3Gi"]))
        if rng.random() < 0.12:
            p.containers[0].requests[DEVICE_RESOURCE] = "1"
        pods.append(p)
    return Problem(instance_types=its, provisioners=provs, pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


# ---------------------------------------------------------------------------------------------------------------- a batch of what-ifs over a snapshot with a limit
WHATIF_SETS = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]


def limited_snapshot():
    """24 nodes, full by pod count but for two, whose provisioner is limited to exactly the cpu its nodes hold: a what-if has the capacity of the nodes it removes to
    open machines with, so the limit decides which types a replacement may be.  Returns (snapshot problem, pod -> node)."""
    from karpenter_core_amd import workloads as W
    its, prov, nodes, bound = W.cluster_snapshot(existing=24, sizes=5, seed=11, spare_pod_slots=2)
    prov.limits = {"cpu": str(int(sum(fake._qty_value(n.capacity["cpu"]) for n in nodes)))}
    return W.snapshot_problem(its, prov, nodes, bound, False)


def run_whatifs(S):
    """The what-ifs flattened one by one are clean by reference and device; the batch form over the same what-ifs says the same; derived on the device -- the
    snapshot's classes, each what-if's own remaining resources -- they give the same flags for the new nodes and the same counters; in at least one the limit
    excludes a type; a claimed result on a derived view is refused.  Returns the summaries of the derived what-ifs."""
    snap, pn = limited_snapshot()
    flats = S.open_whatifs(snap, pn, WHATIF_SETS, derive=False)
    for f in flats:
        f.upload(0)
    S.solve_batch(flats, decode=False)
    plain = [assert_clean(S, f) for f in flats]
    for b, p in zip(S.audit_limits_batch(flats), plain):
        assert np.array_equal(b["pod_flags"], p["pod_flags"]) and np.array_equal(b["node_flags"], p["node_flags"]) and summary(b) == summary(p)
    derived = S.open_whatifs(S.ParsedProblem(snap), pn, WHATIF_SETS, derive=True)
    S.solve_batch_resident(derived)
    got = S.audit_limits_batch(derived)
    assert len(got) == len(WHATIF_SETS)
    new = lambda d: d["node_flags"][len(d["node_flags"]) - d["n_new"]:]      # (a derived what-if numbers its existing nodes by the snapshot's rows)
    for d, p in zip(got, plain):
        assert not d["pod_flags"].any() and not d["node_flags"].any() and len(d["pod_flags"]) == len(p["pod_flags"]), (summary(d), summary(p))
        assert summary(d) == summary(p) and np.array_equal(new(d), new(p)), (summary(d), summary(p))
    assert all(d["limited_templates"] == 1 for d in got) and sum(d["checked"]["NODES"] for d in got) >= 3 and any(d["binding_nodes"] > 0 for d in got), [summary(d) for d in got]
    try:
        derived[0].audit_limits(claimed=flats[0].result_arrays(), pod_seq=np.zeros(len(plain[0]["pod_flags"]), dtype=np.int32))
        code = S.KS_OK
    except S.KSolveError as e:
        code = e.code
    assert code == S.KS_ERR_UNSUPPORTED, code
    out = [summary(d) for d in got]
    for f in flats + derived:
        f.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- shapes where the kernels take another path
TYPE_SHAPES = [1, 64, 65, 130]
NODE_SHAPES = [1, 64, 65, 257]
SHAPE_NAMES = ["T = %d: EXTRA and MISSING decided at bit %d" % (T, T - 1) for T in TYPE_SHAPES] + ["n_m = %d: the edit on the last node" % n for n in NODE_SHAPES] + \
              ["a limited template between two unlimited ones", "12 resource names, the limited one at index >= 8", "R0 negative from the start", "no limited template", "n_new = 0", "P = 1", "limits = {}"]


def last_type_problem(T: int, limit: int) -> Problem:
    """T types; two pods that only the largest holds, one per machine, and a cpu limit: 2T lets the largest in twice, 2T - 1 once."""
    its = fake.instance_types(T)
    return Problem(instance_types=its, provisioners=[fake.provisioner("capped", len(its), limits={"cpu": str(limit)})],
                   pods=[TC._pod("w%d" % i, cpu="%dm" % (T * 1000 - 500), mem="64Mi") for i in range(2)], nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def chain_problem(n: int) -> Problem:
    """n + 1 pods that each fill a two-core machine (two types: 1 and 2 cores), under a cpu limit of 2n: every opening takes 2 cores off, the n-th opens at exactly 2,
    the last pod finds nothing left."""
    its = fake.instance_types(2)
    return Problem(instance_types=its, provisioners=[fake.provisioner("capped", len(its), limits={"cpu": str(2 * n)})],
                   pods=[TC._pod("c%03d" % i, cpu="1500m", mem="64Mi") for i in range(n + 1)], nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def between_problem() -> Problem:
    """taint-free `first` (one-core type only: no pod fits), `capped` (limited), `last`: M = 3 with the limited template in the middle."""
    its = fake.instance_types(6)
    provs = [fake.provisioner("first", weight=30, instance_types=[0]), fake.provisioner("capped", len(its), weight=20, limits={"cpu": "10"}), fake.provisioner("last", len(its), weight=10)]
    return Problem(instance_types=its, provisioners=provs, pods=[TC._pod("p%d" % i, cpu="2500m", mem="1Gi") for i in range(5)], nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def wide_names_problem() -> Problem:
    """Twelve resource names, the limited one the last: nine extended resources behind cpu, memory and pods; a.example/r8 runs with the cores -- type i has i + 1 of it --
    and `capped` limits it to 10 (and the other eight to a thousand, which never binds), so the openings are `capped_problem`'s."""
    names = ["a.example/r%d" % i for i in range(9)]
    its = [fake.new_instance_type("fake-it-%d" % i, dict({"cpu": str(i + 1), "memory": "%dGi" % (2 * (i + 1)), "pods": str(10 * (i + 1))}, **{n: (str(i + 1) if n == names[-1] else "4") for n in names}))
           for i in range(6)]
    pods = [TC._pod("p%d" % i, cpu="2500m", mem="1Gi") for i in range(5)]
    for p in pods:
        for n in names[:-1]:
            p.containers[0].requests[n] = "1"
    return Problem(instance_types=its, provisioners=[fake.provisioner("capped", len(its), weight=10, limits=dict({n: "1000" for n in names[:-1]}, **{names[-1]: "10"})), fake.provisioner("second", len(its), weight=1)],
                   pods=pods, nodes=[], extra_well_known=fake.EXTRA_WELL_KNOWN)


def negative_problem() -> Problem:
    """Three six-core existing nodes of `capped` against a limit of 10: R0 = -8; every pod goes to `second`."""
    pr = capped_problem(pods=3)
    for e in range(3):
        n = C._node("e%d" % e, C.Z1, "0m")
        n.labels[LABEL_PROVISIONER] = "capped"
        pr.nodes.append(n)
    return pr


def run_shapes(S):
    report = []

    def shape(name, make, body, **kw):
        flat = S.FlatProblem(make(), flags=S.KS_FLAG_NO_RR, **kw)
        try:
            flat.solve(decode=False)
            dev = assert_clean(S, flat)
            ok = body(flat, dev)
        except AssertionError as e:
            ok = "%s" % (e,)
        flat.close()
        report.append((name, ok))

    def claim(flat, edit):
        res, seq = _claimable(flat.result_arrays()), np.array(flat.pod_seq(), dtype=np.int32)
        edit(res, seq)
        dev, ref = compare(S, flat, res, seq)
        return flagged(dev["node_flags"]), flagged(dev["pod_flags"])

    def last_type(T):
        def body(flat, dev):
            res = flat.result_arrays()
            assert flat.dims["T"] == T and res["n_new"] == 2 and [_types(res, j) for j in range(2)] == [1 << (T - 1)] * 2 and dev["exact_nodes"] == 2, (flat.dims, dev)
            got = claim(flat, lambda r, s: _set_types(r, 1, 0))      # the walk over the types must reach the one bit to say that it is missing
            assert got == ({1: MISSING}, {}), got
            # one core less of limit: the second pod stays unscheduled, and a claimed second machine cannot have held the largest type
            short = S.FlatProblem(last_type_problem(T, 2 * T - 1), flags=S.KS_FLAG_NO_RR)
            try:
                short.solve(decode=False)
                d2 = assert_clean(S, short)
                r2 = short.result_arrays()
                assert r2["n_new"] == 1 and len(r2["unscheduled"]) == 1 and d2["checked"]["PODS"] == 2, (r2["n_new"], r2["unscheduled"], d2)
                got = claim(short, lambda r, s: _open_copy(r, s, 0, int(r2["unscheduled"][0])))
                assert got == ({1: EXTRA}, {}), got
            finally:
                short.close()
            return True
        return body
    for T, name in zip(TYPE_SHAPES, SHAPE_NAMES):
        shape(name, lambda T=T: last_type_problem(T, 2 * T), last_type(T))

    def chain(n):
        def body(flat, dev):
            res, seq = flat.result_arrays(), flat.pod_seq()
            assert res["n_new"] == n and len(res["unscheduled"]) == 1 and dev["checked"]["NODES"] == n and dev["exact_nodes"] == n and dev["skipped_nodes"] == 0, dev
            j = int(res["pod_node"][int(np.argmax(seq))])      # the node opened last: L_j == U_j == 2 exactly -- the prefix sum crosses lanes, waves and tiles
            assert _types(res, j) == 0x2
            got = claim(flat, lambda r, s: _set_types(r, j, 0))
            assert got == ({j: MISSING}, {}), got
            got = claim(flat, lambda r, s: _open_copy(r, s, j, int(res["unscheduled"][0])))      # one machine more: nothing remained
            assert got == ({n: EXTRA}, {}), got
            return True
        return body
    for n, name in zip(NODE_SHAPES, SHAPE_NAMES[4:8]):
        shape(name, lambda n=n: chain_problem(n), chain(n))

    def between(flat, dev):
        res = flat.result_arrays()
        assert flat.dims["M"] == 3 and [int(x) for x in res["node_tmpl"]] == [1, 1, 2] and dev["limited_templates"] == 1 and dev["exact_nodes"] == 2 and dev["checked"]["PAIRS"] == 1, (res["node_tmpl"], dev)

        def bill(r, s):
            r["node_tmpl"][1] = 2
        got = claim(flat, bill)
        assert got == ({}, {2: LIMIT, 3: LIMIT}), got      # (pod 3 too: with node 1 off its bill capped still had 4 cores at commit 3)
        return True
    shape(SHAPE_NAMES[8], between_problem, between)

    def wide(flat, dev):
        names = flat.resource_names()
        assert flat.dims["R"] == 12 and names.index("a.example/r8") >= 8, names
        res = flat.result_arrays()
        assert [_types(res, j) for j in range(3)] == [0x20, 0x0C, 0x20] and dev["exact_nodes"] == 2 and dev["binding_nodes"] >= 1, dev
        got = claim(flat, lambda r, s: _set_types(r, 1, 0x1C))
        assert got == ({1: EXTRA}, {}), got
        got = claim(flat, lambda r, s: _set_types(r, 1, 0x04))
        assert got == ({1: MISSING}, {}), got
        return True
    shape(SHAPE_NAMES[9], wide_names_problem, wide)

    def negative(flat, dev):
        res = flat.result_arrays()
        E = flat.dims["E"]
        assert E == 3 and [int(x) for x in res["node_tmpl"]] == [1, 1] and dev["checked"]["NODES"] == 0 and dev["checked"]["PAIRS"] == 1, (res["node_tmpl"], dev)

        def bill(r, s):
            r["node_tmpl"][0] = 0
        got = claim(flat, bill)
        assert got[0] == {E: EXTRA}, got
        return True
    shape(SHAPE_NAMES[10], negative_problem, negative)
    shape(SHAPE_NAMES[11], lambda: TC.plain(3), lambda flat, dev: True if dev["limited_templates"] == 0 and dev["checked"] == {"SEQ": 3, "NODES": 0, "PODS": 0, "PAIRS": 0} and dev["skipped_pods"] == 0 else str(dev))

    def no_new(flat, dev):
        return True if dev["n_new"] == 0 and dev["limited_templates"] == 1 and dev["checked"] == {"SEQ": 2, "NODES": 0, "PODS": 2, "PAIRS": 1} else str(dev)

    def no_new_problem():
        pr = capped_problem(pods=2, second=False)
        pr.nodes.append(TC._roomy("e0", C.Z1))
        return pr
    shape(SHAPE_NAMES[12], no_new_problem, no_new)

    def one_pod(flat, dev):
        assert flat.dims["P"] == 1 and dev["checked"] == {"SEQ": 1, "NODES": 1, "PODS": 1, "PAIRS": 1} and dev["exact_nodes"] == 1, dev
        got = claim(flat, lambda r, s: _set_types(r, 0, 0x30))
        assert got == ({0: MISSING}, {}), got      # the three- and four-core types hold the pod as well
        return True
    shape(SHAPE_NAMES[13], lambda: capped_problem(pods=1, second=False), one_pod)

    def empty_limits(flat, dev):
        res = flat.result_arrays()
        assert dev["limited_templates"] == 1 and dev["binding_nodes"] == 0 and dev["exact_nodes"] == res["n_new"], dev
        got = claim(flat, lambda r, s: _set_types(r, 1, 0x04))      # limited with no limited resource: the second node keeps every type that holds its pod
        assert got == ({1: MISSING}, {}), got
        return True

    def empty_limits_problem():
        pr = capped_problem(pods=3, second=False)
        pr.provisioners[0].limits = {}
        return pr
    shape(SHAPE_NAMES[14], empty_limits_problem, empty_limits)
    assert [r[0] for r in report] == SHAPE_NAMES
    return report
