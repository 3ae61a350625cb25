"""What tests/test_audit_stages.py (on the lane-fibre emulator) and tests/test_audit_stages_gpu.py (on the device) share: the comparison of the audit's seventh pass
with its reference (tests/audit_stages_ref.py, over tests/audit_harness.py's Pass), a small seeded family of problems in which pods really RELAX -- few committed
cases do --, the tamper matrix and the shapes at which the kernels take another path.  Every function takes the scheduler module `S` it is to go through (the HIP
libraries' or the emulator's)."""
import numpy as np

import audit_cases as C
import audit_firstfit_cases as FC
import audit_harness as H
import audit_stages_ref as SR
import audit_topo_cases as TC
from audit_harness import _claimable, flagged
from karpenter_core_amd import fake
from karpenter_core_amd.model import LABEL_INSTANCE_TYPE, LABEL_ZONE, Expr, PreferredTerm, Problem

B = SR.BITS
Z1, Z2, Z3 = C.Z1, C.Z2, C.Z3
NOWHERE = "test-zone-9"      # a zone nothing offers
_COUNTERS = ("pairs_existing", "pairs_template", "unscheduled_examined", "used_classes")      # the reference's alone: what the soundness gate counts beyond the out struct


class StagesPass(H.Pass):
    """tests/audit_harness.py's Pass for the seventh pass.  Pass finds the binding's struct by a table of the six passes of scheduler._AUDIT_PASSES; the seventh stands
    beside that table, so it is constructed as the pass whose shape it has -- the fourth -- and then given its own names."""

    def __init__(self):
        super().__init__("firstfit", SR, SR.BITS, checked=SR.CHECKED, gives=None, counters=("admitting_pairs", "skipped_pods"),
                         summary=(("admitting", "admitting_pairs"), ("skipped", "skipped_pods")) + H._PLACED, pods_identity=True)
        self.name, self.method, self.stem, self.batch, self.out = "stages", "audit_stages", "audit_stages", "audit_stages_batch", "_AuditStagesOut"


D = StagesPass()
compare, assert_clean, summary = D.compare, D.assert_clean, D.summary


def summary_with_reference(dev, ref):
    """summary(dev) plus the reference's own counters: what the soundness gate sums."""
    return dict(summary(dev), **{k: int(ref[k]) for k in _COUNTERS})


def _prefer(*terms):
    """preferred node affinity: (weight, key, value) each -- Relax drops the heaviest first (preferences.go:58-71), one stage per term"""
    return [PreferredTerm(w, [Expr(k, "In", [v])]) for w, k, v in terms]


def _either(*terms):
    """required node affinity of several OR'd terms, (key, value) each: Relax drops the first while more than one is left (preferences.go:73-87), so stage j + 1
    carries the NEXT term instead of the one before -- a chain whose later class is no relaxation of the earlier one"""
    return [[Expr(k, "In", [v])] for k, v in terms]


def _team_node(name, zone, cpu):
    n = C._node(name, zone, cpu)
    n.labels["team"] = "a"      # a custom label no provisioner defines: a preference for it is satisfiable on this node alone
    return n


# ---------------------------------------------------------------------------------------------------------------- the family: pods that relax
FAMILY = [("relax_%d_%s" % (seed, "existing" if ex else "empty"), {"seed": seed, "existing": ex}) for seed in (1, 2, 3) for ex in (True, False)]


def relax_problem(seed: int, existing: bool = True, scale: int = 1) -> Problem:
    """Pods whose preferences cannot all hold.  nowhere-*: preferred affinity to a zone nothing offers (chains of 2).  typed-*: two preferences, a zone nothing offers
    and an instance type nothing lists (chains of 3).  fill-*: a preference for the label `team=a`, which only the small existing node e0 carries: the first few
    land there unrelaxed, the others relax once it is full (without existing nodes: all relax).  keep-*: a preference that holds (never relax).  long-0: 34
    preferences for instance types nothing lists (a chain of 35 stages, walked to its end).  giant-*: a preference nothing satisfies on a pod no machine holds
    (unscheduled after a full chain).  either-*: two OR'd REQUIRED terms of which only the second can hold (they relax once, to a class that is no relaxation of
    the first); first-*: the same with the terms swapped (never relax).  plain-*: no preference.  scale: the pods of every kind, times this."""
    rs = np.random.RandomState(4200 + seed)
    its = fake.instance_types(6)
    cpu = lambda: "%dm" % [100, 200, 300][int(rs.randint(3))]
    n = 3 * scale + int(rs.randint(3))
    pods = [TC._pod("nowhere-%04d" % i, cpu=cpu(), preferred_affinity=_prefer((10, LABEL_ZONE, NOWHERE))) for i in range(n)]
    pods += [TC._pod("typed-%04d" % i, cpu=cpu(), preferred_affinity=_prefer((20, LABEL_ZONE, NOWHERE), (10, LABEL_INSTANCE_TYPE, "fake-it-99"))) for i in range(n)]
    pods += [TC._pod("fill-%04d" % i, cpu="300m", preferred_affinity=_prefer((5, "team", "a"))) for i in range(n + 2)]
    pods += [TC._pod("keep-%04d" % i, cpu=cpu(), preferred_affinity=_prefer((5, LABEL_ZONE, [Z1, Z2, Z3][int(rs.randint(3))]))) for i in range(n)]
    pods += [TC._pod("long-0", cpu="150m", preferred_affinity=_prefer(*[(100 - i, LABEL_INSTANCE_TYPE, "no-type-%02d" % i) for i in range(34)]))]
    pods += [TC._pod("giant-%d" % i, cpu="500", preferred_affinity=_prefer((10, LABEL_ZONE, NOWHERE))) for i in range(1 + seed % 2)]
    pods += [TC._pod("either-%04d" % i, cpu=cpu(), required_affinity=_either((LABEL_ZONE, NOWHERE), (LABEL_ZONE, [Z1, Z2, Z3][i % 3]))) for i in range(n)]
    pods += [TC._pod("first-%04d" % i, cpu=cpu(), required_affinity=_either((LABEL_ZONE, [Z1, Z2, Z3][i % 3]), (LABEL_ZONE, NOWHERE))) for i in range(2)]
    pods += [TC._pod("plain-%04d" % i, cpu=cpu()) for i in range(n)]
    nodes = [_team_node("e0", Z1, "1"), C._node("e1", Z2, "2"), C._node("e2", Z3, "500m")] if existing else []
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=pods, nodes=nodes, extra_well_known=fake.EXTRA_WELL_KNOWN)


def relax_snapshot(existing: int = 24, seed: int = 11):
    """A cluster snapshot (workloads.cluster_snapshot) whose bound pods partly carry preferences nothing satisfies: the pods of a removed node relax before they
    settle.  Returns (snapshot problem, pod_node) for scheduler.open_whatifs."""
    from karpenter_core_amd import workloads as W
    its, prov, nodes, bound = W.cluster_snapshot(existing=existing, sizes=5, seed=seed)
    rs = np.random.RandomState(700 + seed)
    for pods in bound:
        for p in pods:
            r = rs.rand()
            if r < 0.3:
                p.preferred_affinity = _prefer((10, LABEL_ZONE, NOWHERE))
            elif r < 0.4:
                p.preferred_affinity = _prefer((20, LABEL_ZONE, NOWHERE), (10, LABEL_INSTANCE_TYPE, "no-such-type"))
    return W.snapshot_problem(its, prov, nodes, bound, False)


# ---------------------------------------------------------------------------------------------------------------- the tamper matrix
PODS = ["giant", "plain_a", "plain_b", "team_a", "team_b", "zonal_a", "zonal_b", "either_t", "either_z"]
TAMPER_NAMES = ["(a) a pod on the existing node its preference names, claimed one stage on", "(a) a pod on the machine its preferred zone opened, claimed one stage on",
                "(b) the same existing-node pod claimed unscheduled at the end of its chain", "(b) the same new-node pod claimed unscheduled, its node's requests lowered",
                "(b) a pod of two required terms on the existing node its first term names, claimed unscheduled under its second",
                "(b) a pod of two required terms on the machine its first term opened, claimed unscheduled under its second, the node's requests lowered",
                "(c) an unscheduled pod claimed one stage short of its chain", "(d) two pods given one commit number", "(e) a stage past the chain", "(e) a negative stage"]
SILENT = TAMPER_NAMES[:2] + TAMPER_NAMES[4:6]      # the edits all six earlier passes let through: one per bit of (a) and of (b)
E0, E1 = 0, 1


def tamper_problem() -> Problem:
    """Two existing nodes with five cores to spare -- e0 in zone 1 labelled team=a, e1 in zone 2 --, one provisioner without limits, seven types (the last holds 96
    cores).  team_a / team_b prefer team=a: on e0 at stage 0.  zonal_a / zonal_b (8 cores each: no existing node holds one) prefer zone 3: one machine of the large
    type there, at stage 0.  plain_a / plain_b: on e0.  giant (500 cores) prefers a zone nothing offers: relaxed to the end of its chain, unscheduled.  either_t REQUIRES team=a or, failing that, a zone nothing offers: on e0 at stage 0; either_z (8 cores) requires
    zone 3 or that zone: on the machine in zone 3 at stage 0.  Their second stage is admitted nowhere -- it is no relaxation of the first."""
    its = fake.instance_types(6) + [fake.new_instance_type("huge", {"cpu": "96", "memory": "256Gi", "pods": "200"})]
    pods = [TC._pod("giant", cpu="500", preferred_affinity=_prefer((10, LABEL_ZONE, NOWHERE))), TC._pod("plain_a"), TC._pod("plain_b"),
            TC._pod("team_a", preferred_affinity=_prefer((5, "team", "a"))), TC._pod("team_b", preferred_affinity=_prefer((5, "team", "a"))),
            TC._pod("zonal_a", cpu="8", mem="1Gi", preferred_affinity=_prefer((5, LABEL_ZONE, Z3))), TC._pod("zonal_b", cpu="8", mem="1Gi", preferred_affinity=_prefer((5, LABEL_ZONE, Z3))),
            TC._pod("either_t", required_affinity=_either(("team", "a"), (LABEL_ZONE, NOWHERE))), TC._pod("either_z", cpu="8", mem="1Gi", required_affinity=_either((LABEL_ZONE, Z3), (LABEL_ZONE, NOWHERE)))]
    assert [p.uid for p in pods] == PODS
    return Problem(instance_types=its, provisioners=[fake.provisioner("open", len(its))], pods=pods, nodes=[_team_node("e0", Z1, "5"), C._node("e1", Z2, "5")],
                   extra_well_known=fake.EXTRA_WELL_KNOWN)


def check_genuine(res, seq) -> dict:
    pod = {n: i for i, n in enumerate(PODS)}
    where = {n: int(res["pod_node"][i]) for n, i in pod.items()}
    stage = {n: int(res["pod_stage"][i]) for n, i in pod.items()}
    assert res["n_existing"] == 2 and res["n_new"] == 1 and list(res["unscheduled"]) == [pod["giant"]], (res["n_new"], res["unscheduled"])
    assert [where[n] for n in PODS] == [-1, E0, E0, E0, E0, 2, 2, E0, 2], where
    assert [stage[n] for n in PODS] == [1, 0, 0, 0, 0, 0, 0, 0, 0], stage
    assert sorted(int(s) for s in seq if s >= 0) == list(range(8)) and seq[pod["giant"]] == -1, seq
    return pod


def _unschedule(r, s, q):
    """pod q claimed unscheduled: off its node, out of the commit order, into the list"""
    r["pod_node"][q] = -1
    s[s > s[q]] -= 1
    s[q] = -1
    r["unscheduled"] = np.array(sorted(list(r["unscheduled"]) + [q]), dtype=np.int32)


def tampers(res, seq, prob):
    """[(name, edited copy of `res`, edited copy of `seq`, {pod: bits} -- exactly these flags, on exactly these pods)]"""
    pod = check_genuine(res, seq)
    R = prob["R"]
    out = []

    def case(name, want):
        r, s = _claimable(res), np.array(seq, dtype=np.int32)
        out.append((name, r, s, want))
        return r, s

    def lower(r, q):
        """the one machine's Requests without pod q's: the daemon overhead plus the pods that stay"""
        c = int(prob["stage_cls"][int(prob["pod_stage_off"][q])])
        req = np.asarray(r["node_requests"], dtype=np.int64).reshape(-1, R).copy()
        req[0] -= prob["cls_requests"][c * R:(c + 1) * R].astype(np.int64)
        r["node_requests"] = req.reshape(-1)

    r, s = case(TAMPER_NAMES[0], {pod["team_a"]: B["STAGE_EXISTING"]})      # no provisioner defines `team`: no fresh machine admits the earlier stage, e0 does
    r["pod_stage"][pod["team_a"]] = 1
    r, s = case(TAMPER_NAMES[1], {pod["zonal_a"]: B["STAGE_TEMPLATE"]})     # e0 and e1 are in other zones; a fresh machine in zone 3 admits the earlier stage
    r["pod_stage"][pod["zonal_a"]] = 1
    r, s = case(TAMPER_NAMES[2], {pod["team_b"]: B["STAGE_EXISTING"]})
    r["pod_stage"][pod["team_b"]] = 1
    _unschedule(r, s, pod["team_b"])
    q = pod["zonal_b"]
    r, s = case(TAMPER_NAMES[3], {q: B["STAGE_TEMPLATE"]})
    lower(r, q)
    r["pod_stage"][q] = 1
    _unschedule(r, s, q)
    # (b) where the later class is NO relaxation of the earlier one: the second required term is admitted nowhere, so the fourth pass, which asks about the claimed
    # stage alone, has nothing to say about the unscheduled pod -- and the first term's class is admitted where the pod genuinely sat
    r, s = case(TAMPER_NAMES[4], {pod["either_t"]: B["STAGE_EXISTING"]})
    r["pod_stage"][pod["either_t"]] = 1
    _unschedule(r, s, pod["either_t"])
    q = pod["either_z"]
    r, s = case(TAMPER_NAMES[5], {q: B["STAGE_TEMPLATE"]})
    lower(r, q)
    r["pod_stage"][q] = 1
    _unschedule(r, s, q)
    r, s = case(TAMPER_NAMES[6], {pod["giant"]: B["STAGE_UNRELAXED"]})
    r["pod_stage"][pod["giant"]] = 0
    r, s = case(TAMPER_NAMES[7], {pod["team_a"]: B["SEQ"], pod["plain_a"]: B["SEQ"]})
    r["pod_stage"][pod["team_a"]] = 1      # (would be STAGE_EXISTING: a pod that fails SEQ is not examined)
    s[pod["team_a"]] = s[pod["plain_a"]]
    r, s = case(TAMPER_NAMES[8], {})
    r["pod_stage"][pod["team_a"]] = 1 << 30
    r, s = case(TAMPER_NAMES[9], {})
    r["pod_stage"][pod["giant"]] = -5
    assert [x[0] for x in out] == TAMPER_NAMES
    return out


def earlier_passes_silent(flat, claimed, s):
    """True, or which of the six earlier passes flags the claimed result (the gate: all six in one call)"""
    g = flat.audit_gate(claimed, s)
    if g["clean"]:
        return True
    return "an earlier pass flags the edit: %s" % ({w: {k: v for k, v in d[0].items() if k.endswith("bit_count")} for w, d in g["passes"].items() if d[0]["n_pods_flagged"] or d[0].get("n_nodes_flagged")},)


def run_tamper_matrix(S, flags: int = 0):
    """(flags: the FlatProblem's, KS_FLAG_NO_RR for the other pack kernel.)  Solve `tamper_problem`, audit the genuine result (clean, and not for lack of anything to examine) and every edit through the claimed form; returns
    [(name, True or what differs)]."""
    flat = S.FlatProblem(tamper_problem(), flags=flags)
    flat.solve(decode=False)
    dev = assert_clean(S, flat)
    assert dev["checked"] == {"SEQ": 8, "PODS": 1, "STAGES": 1, "PAIRS": 3} and dev["admitting_pairs"] == 0 and dev["skipped_pods"] == 8, dev      # giant's stage 0 against e0, e1 and the template
    res, seq, prob = flat.result_arrays(), flat.pod_seq(), SR.problem_arrays(S, flat)
    report = []
    for name, claimed, s, want in tampers(res, seq, prob):
        try:
            dev, ref = compare(S, flat, claimed, s)
            got = flagged(dev["pod_flags"])
            ok = True if got == want else "flags %s, expected %s" % (got, want)
        except AssertionError as e:
            ok = "device and reference differ: %s" % (e,)
        if ok is True and name in SILENT:      # the hole this pass closes
            ok = earlier_passes_silent(flat, claimed, s)
        if ok is True and name.startswith("(b)") and name not in SILENT:      # the edit is consistent: the first pass finds nothing in it
            first = flat.audit(claimed)
            if first["n_pods_flagged"] or first["n_nodes_flagged"]:
                ok = "the first pass flags the edit: %s %s" % (first["pod_bit_count"], first["node_bit_count"])
        if ok is True and name.startswith("(e)"):      # not examined, nothing addressed: the pod is skipped, and what was examined before still is
            skipped = 8 if "past" in name else 9      # (team_a had no earlier stage to lose; giant's leaves with its stage)
            if dev["skipped_pods"] != skipped or dev["checked"]["PODS"] != 9 - skipped:
                ok = "skipped %d pods, expected %d" % (dev["skipped_pods"], skipped)
        report.append((name, ok))
    flat.close()
    return report


# ---------------------------------------------------------------------------------------------------------------- shapes where the kernels take another path
TYPE_SHAPES = FC.TYPE_SHAPES
NODE_SHAPES = [(65, 0), (65, 63), (257, 0), (257, 255)]
SHAPE_NAMES = ["P = 1", "a pod with a one-stage chain: nothing to examine", "no pod relaxed at all: the early-out", "33 stages, the only admitting stage 0", "33 stages, the only admitting stage k - 1",
               "1 used class", "257 used classes"] + ["T = %d: the only admitting type at bit %d" % ts for ts in TYPE_SHAPES] + ["E = 0"] + \
              ["E = %d: the only admitting node at index %d" % ns for ns in NODE_SHAPES] + ["two templates of which only the second, unlimited one admits", "12 resource names"]


def _open(its, pods, nodes=(), provs=None):
    return Problem(instance_types=its, provisioners=provs or [fake.provisioner("open", len(its))], pods=pods, nodes=list(nodes), extra_well_known=fake.EXTRA_WELL_KNOWN)


def long_chain(first: bool) -> Problem:
    """One pod with 32 preferences -- 33 stages --, of which only the first (heaviest), or only the last, can hold: a zone that exists among instance types that do not."""
    terms = [(100 - i, LABEL_ZONE, Z2) if i == (0 if first else 31) else (100 - i, LABEL_INSTANCE_TYPE, "no-type-%02d" % i) for i in range(32)]
    return _open(fake.instance_types(4), [TC._pod("chained", preferred_affinity=_prefer(*terms))])


def many_relaxed(n: int, nodes: int = 2) -> Problem:
    """n pods of n different requests: all but the last prefer a zone nothing offers and relax; the last prefers zone 1 and lands on e0 unrelaxed.  `nodes` roomy
    existing nodes, in zones 1 and 2 by turns."""
    pods = [TC._pod("c%03d" % i, cpu="%dm" % (i + 1), preferred_affinity=_prefer((5, LABEL_ZONE, NOWHERE if i < n - 1 else Z1))) for i in range(n)]
    return _open(fake.instance_types(4), pods, [TC._roomy("e%d" % e, Z2 if e % 2 else Z1) for e in range(nodes)])


def one_type_fits(T: int) -> Problem:
    """tests/audit_firstfit_cases.py's ladder of T types and its one pod that only the largest holds, with a preference that holds"""
    pr = FC.one_type_fits(T)
    pr.pods[0].preferred_affinity = _prefer((5, LABEL_ZONE, Z1))
    return pr


def one_node_fits(E: int, at: int) -> Problem:
    """E existing nodes labelled team=a, all full but node `at`, and one pod that prefers the label"""
    nodes = [_team_node("e%03d" % i, Z1, "5" if i == at else "50m") for i in range(E)]
    return _open(fake.instance_types(4), [TC._pod("p0", preferred_affinity=_prefer((5, "team", "a")))], nodes)


def second_template() -> Problem:
    its = fake.instance_types(4)
    provs = [fake.provisioner("capped", len(its), weight=10, limits={"cpu": "100"}), fake.provisioner("open", len(its), weight=1)]
    return _open(its, [TC._pod("p0", preferred_affinity=_prefer((5, LABEL_ZONE, Z2)))], provs=provs)


def wide_problem() -> Problem:
    pr = FC.wide_problem()
    pr.pods = list(pr.pods) + [TC._pod("zz-relax-%d" % i, cpu="10m", mem="8Mi", preferred_affinity=_prefer((5, LABEL_ZONE, NOWHERE))) for i in range(3)]
    return pr


def run_shapes(S, flags: int = 0):
    """(flags: the FlatProblems', KS_FLAG_NO_RR for the other pack kernel.)  [(name, True or what differs)] -- each shape solved (clean by device and reference) and, where it says so, one claimed edit."""
    report = []

    def shape(name, make, body):
        flat = S.FlatProblem(make(), flags=flags)
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
        return dev, flagged(ref["pod_flags"])

    def stage_on(p, want, checked=None):
        """pod p, genuine at stage k, claimed at stage k + 1: `want` on it alone"""
        def body(flat, dev):
            def edit(r, s):
                r["pod_stage"][p] += 1
            d, got = claim(flat, edit)
            assert got == {p: want}, got
            assert checked is None or d["checked"] == checked, d["checked"]
            return True
        return body
    EX, TM = B["STAGE_EXISTING"], B["STAGE_TEMPLATE"]
    nothing = lambda n: {"SEQ": n, "PODS": 0, "STAGES": 0, "PAIRS": 0}
    shape(SHAPE_NAMES[0], lambda: _open(fake.instance_types(4), [TC._pod("p0", preferred_affinity=_prefer((5, LABEL_ZONE, NOWHERE)))]),
          lambda flat, dev: True if flat.dims["P"] == 1 and dev["checked"] == {"SEQ": 1, "PODS": 1, "STAGES": 1, "PAIRS": 1} and dev["admitting_pairs"] == 0 else str(dev))
    shape(SHAPE_NAMES[1], lambda: TC.plain(1), lambda flat, dev: True if dev["checked"] == nothing(1) and dev["skipped_pods"] == 1 else str(dev))
    shape(SHAPE_NAMES[2], lambda: TC.plain(3, True), lambda flat, dev: True if dev["checked"] == nothing(3) and dev["skipped_pods"] == 3 and dev["admitting_pairs"] == 0 and dev["n_placed"] == 3 else str(dev))

    def chain(first):
        def body(flat, dev):
            res = flat.result_arrays()
            k = 0 if first else 31
            assert [int(x) for x in res["pod_stage"]] == [k] and dev["checked"]["STAGES"] == k, (res["pod_stage"], dev)

            def edit(r, s):
                r["pod_stage"][0] = 32
            d, got = claim(flat, edit)
            assert got == {0: TM} and d["checked"]["STAGES"] == 32 and d["admitting_pairs"] == 1, (got, d)      # 32 stages walked, one class of them admitted by the one template
            return True
        return body
    shape(SHAPE_NAMES[3], lambda: long_chain(True), chain(True))
    shape(SHAPE_NAMES[4], lambda: long_chain(False), chain(False))
    shape(SHAPE_NAMES[5], lambda: many_relaxed(2), lambda flat, dev: True if dev["checked"] == {"SEQ": 2, "PODS": 1, "STAGES": 1, "PAIRS": 3} else str(dev))

    def classes_257(flat, dev):
        assert dev["checked"] == {"SEQ": 257, "PODS": 256, "STAGES": 256, "PAIRS": 256 * 3} and dev["admitting_pairs"] == 0, dev
        return stage_on(256, EX | TM, {"SEQ": 257, "PODS": 257, "STAGES": 257, "PAIRS": 257 * 3})(flat, dev)      # the class past the scan tile finds its own row of the first_* tables
    shape(SHAPE_NAMES[6], lambda: many_relaxed(257), classes_257)
    for (T, bit), name in zip(TYPE_SHAPES, SHAPE_NAMES[7:11]):
        shape(name, lambda T=T: one_type_fits(T), stage_on(0, TM, {"SEQ": 1, "PODS": 1, "STAGES": 1, "PAIRS": 1}))      # the walk over the types must reach the one bit to say so
    shape(SHAPE_NAMES[11], lambda: one_type_fits(4), lambda flat, dev: True if flat.dims["E"] == 0 and dev["checked"] == nothing(1) else str(dev))

    def only_node(E, at):
        def body(flat, dev):
            assert flat.dims["E"] == E and [int(x) for x in flat.result_arrays()["pod_node"]] == [at], flat.result_arrays()["pod_node"]
            return stage_on(0, EX, {"SEQ": 1, "PODS": 1, "STAGES": 1, "PAIRS": E + 1})(flat, dev)      # the minimum over the existing nodes crosses lanes, waves and workgroups
        return body
    for (E, at), name in zip(NODE_SHAPES, SHAPE_NAMES[12:16]):
        shape(name, lambda E=E, at=at: one_node_fits(E, at), only_node(E, at))
    shape(SHAPE_NAMES[16], second_template, lambda flat, dev: stage_on(0, TM, {"SEQ": 1, "PODS": 1, "STAGES": 1, "PAIRS": 1})(flat, dev) if flat.dims["M"] == 2 else str(flat.dims))
    shape(SHAPE_NAMES[17], wide_problem, lambda flat, dev: True if flat.dims["R"] == 12 and dev["checked"]["STAGES"] >= 3 and dev["checked"]["PAIRS"] > 0 else str((flat.dims, dev)))
    assert [r[0] for r in report] == SHAPE_NAMES
    return report


# ---------------------------------------------------------------------------------------------------------------- what-ifs derived on the device
RELAX_WHATIF_SETS = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]


def derived_whatifs(S):
    """`relax_snapshot`'s what-ifs with removed nodes, flattened one by one (clean by reference and device) and derived on the device as ONE batch (clean, and counting
    what its flattened twin counts).  Returns ([summary with the reference's counters] of the flattened, [summary] of the derived)."""
    snap, pod_node = relax_snapshot()
    parsed = S.ParsedProblem(snap)
    flats = S.open_whatifs(parsed, pod_node, RELAX_WHATIF_SETS, derive=False)
    S.solve_batch(flats, decode=False)
    plain = []
    for f in flats:
        dev, ref = compare(S, f)
        assert not dev["pod_flags"].any() and dev["n_pods_flagged"] == 0, dev["pod_bit_count"]
        plain.append(summary_with_reference(dev, ref))
    batch = S.audit_stages_batch(flats)      # the batch form over flattened problems says what one call each said
    for b, p in zip(batch, plain):
        assert summary(b) == {k: v for k, v in p.items() if k not in _COUNTERS}, (summary(b), p)
    derived = S.open_whatifs(parsed, pod_node, RELAX_WHATIF_SETS, derive=True)
    S.solve_batch_resident(derived)
    got = S.audit_stages_batch(derived)
    assert len(got) == len(RELAX_WHATIF_SETS)
    for d, p in zip(got, plain):
        assert not d["pod_flags"].any() and d["n_pods_flagged"] == 0, d["pod_bit_count"]
        assert summary(d) == {k: v for k, v in p.items() if k not in _COUNTERS}, (summary(d), p)
    assert sum(d["checked"]["STAGES"] for d in got) > 0 and sum(d["checked"]["PAIRS"] for d in got) > 0, [summary(d) for d in got]
    try:      # a claimed result on a derived view
        derived[0].audit_stages(flats[0].result_arrays(), np.zeros(flats[0].dims["P"], dtype=np.int32))
        refused = None
    except S.KSolveError as e:
        refused = e.code
    assert refused == S.KS_ERR_UNSUPPORTED, refused
    for f in flats + derived:
        f.close()
    return plain, [summary(d) for d in got]
