"""What the tests of the audit's WIDE gate share (tests/test_audit_gate_ex*.py): tests/audit_gate_checks.py for eight passes.  The comparison of `scheduler.audit_gate`
naming "stages" and "reasons" with the EIGHT passes' own calls over the same results -- the reference here: the calls are unchanged by the gate and pinned against the
literal references by their own suites --, the wide gate against the old one over a mask of the six, and a recorder of its own that puts the comparison behind every
call the two passes' cases modules make (tests/audit_stages_cases.py, tests/audit_reasons_cases.py).  Every function takes the scheduler module `S` it is to go
through (the HIP libraries' or the emulator's)."""
import numpy as np

import audit_gate_checks as G

POISON = G.POISON
# a new pass alone, each | first + stages + reasons: in the claimed form both side arrays travel in one upload | firstfit + stages: the fourth pass's kernels back to back in two roles
EX_MASKS = (["stages"], ["reasons"], ["audit", "stages", "reasons"], ["firstfit", "stages"])
SIX_MASKS = (None, ["firstfit"], ["audit", "firstfit", "hostfit"])      # within the six: the wide gate and the old one must answer alike


def eight_calls(S, flats, claimed=None, pod_seq=None, passes=None):
    """{pass: [one dict per problem]} through the passes' own calls (`scheduler._audit`), in mask order."""
    audit = getattr(S, "_audit_unrecorded", S._audit)
    names = [w for w in S.AUDIT_GATE_ALL if passes is None or w in passes]
    return {w: audit(w, flats, claimed, pod_seq if S._AUDIT_PASSES_EX[w]["seq"] else None) for w in names}


def expected_findings(S, eight):
    """The non-zero entries of the passes' flag tables in the gate's order: by pass as AUDIT_GATE_ALL has them, by problem, pods before nodes, by index."""
    rec = []
    for k, w in enumerate(S.AUDIT_GATE_ALL):
        for i, d in enumerate(eight.get(w, [])):
            for t, key in enumerate(("pod_flags", "node_flags")):
                if key in d:
                    rec += [(i, k << 8 | t, int(x), int(d[key][x])) for x in np.nonzero(d[key])[0]]
    return np.array(rec, dtype=S.AUDIT_FINDING) if rec else np.zeros(0, dtype=S.AUDIT_FINDING)


def same_totals(S, gate, eight):
    """Every totals field of every requested pass is what the pass's own call returned (tests/audit_gate_checks.py's rule: every key but the flag arrays, the times and
    the bit counts the binding counts from the rows where the C struct holds none), and "passes" is in mask order."""
    assert list(gate["passes"]) == [w for w in S.AUDIT_GATE_ALL if w in eight], (list(gate["passes"]), list(eight))
    for w, rows in eight.items():
        assert len(gate["passes"][w]) == len(rows), w
        for i, (g, d) in enumerate(zip(gate["passes"][w], rows)):
            want = {k: v for k, v in d.items() if k not in ("pod_flags", "node_flags", "ms")}
            derived = set(want) - set(g)
            assert derived <= {"pod_bit_count"} and (not derived or not hasattr(S._AUDIT_PASSES_EX[w]["Out"](), "pod_bit_count")), (w, derived)
            for k in derived:
                del want[k]
            assert g == want, (w, i, {k: (g.get(k), want.get(k)) for k in set(g) | set(want) if g.get(k) != want.get(k)})


def wide_as_old(S, flats, claimed=None, pod_seq=None, masks=SIX_MASKS, cap=4096):
    """A mask within the six through the wide gate's entry points and through the old ones: the same totals, the same findings' bytes, the same counts."""
    for names in masks:
        old = S.audit_gate(flats, names, cap, claimed, pod_seq)
        new = S.audit_gate(flats, names, cap, claimed, pod_seq, wide=True)
        assert list(new["passes"]) == list(old["passes"]) and new["passes"] == old["passes"], names
        assert new["findings"].tobytes() == old["findings"].tobytes() and (new["n_findings"], new["truncated"], new["clean"]) == (old["n_findings"], old["truncated"], old["clean"]), names


def gate_against_calls(S, flats, claimed=None, pod_seq=None, masks=(None,) + EX_MASKS, cap=4096, six=True):
    """The wide gate over `flats` (or `claimed` for flats[0]) against the eight calls: totals, findings, `clean`, twice with equal bytes -- for all eight passes and for
    each sub-mask -- and (six) against the old gate over a mask of the six.  Returns (the eight calls' dicts, the gate's dict with all eight passes)."""
    if claimed is not None and pod_seq is None:
        pod_seq = G.pod_order_seq(claimed, flats[0].dims["P"])
    eight = eight_calls(S, flats, claimed, pod_seq)
    full = None
    for names in masks:
        part = eight if names is None else {w: eight[w] for w in S.AUDIT_GATE_ALL if w in names}
        runs = [S.audit_gate(flats, list(S.AUDIT_GATE_ALL) if names is None else names, cap, claimed, pod_seq) for _ in range(2)]
        g = runs[0]
        same_totals(S, g, part)
        want = expected_findings(S, part)
        assert g["n_findings"] == len(want) and not g["truncated"], (names, g["n_findings"], len(want), g["truncated"])
        assert g["findings"].tobytes() == want.tobytes(), (names, g["findings"][:8], want[:8])
        assert g["clean"] == (len(want) == 0) == all(not d[k].any() for rows in part.values() for d in rows for k in ("pod_flags", "node_flags") if k in d)
        assert runs[1]["findings"].tobytes() == g["findings"].tobytes() and runs[1]["passes"] == g["passes"] and runs[1]["n_findings"] == g["n_findings"], names
        if names is None:
            full = g
    if six:
        wide_as_old(S, flats, claimed, pod_seq, masks=(None,))
    return eight, full


class Recorder:
    """Puts `gate_against_calls` behind every call of a pass that goes through `S._audit` -- the methods of FlatProblem and the batch functions, which is how the cases
    modules audit.  `seen`: [(pass, problems, claimed?, findings of all eight, findings of passes 6 and 7)], `gates`: the wide gate's dict of each; a call the pass
    refuses raises before the gate is asked."""

    def __init__(self, S, masks=(None,)):
        self.S, self.masks, self.seen, self.gates, self.busy = S, masks, [], [], False
        S._audit_unrecorded = S._audit
        S._audit = self

    def __call__(self, what, flats, claimed=None, pod_seq=None):
        res = self.S._audit_unrecorded(what, flats, claimed, pod_seq)
        if not self.busy and len(flats):
            self.busy = True
            try:
                eight, g = gate_against_calls(self.S, flats, claimed, pod_seq, masks=self.masks)
                self.seen.append((what, len(flats), claimed is not None, g["n_findings"], int((g["findings"]["where"] >> 8 >= 6).sum())))
                self.gates.append(g)
            finally:
                self.busy = False
        return res

    def remove(self):
        self.S._audit = self.S._audit_unrecorded
        del self.S._audit_unrecorded


def new_pass_findings(g):
    """{pass: {pod: flags}} of the wide gate's findings under passes 6 and 7"""
    out = {6: {}, 7: {}}
    for x in g["findings"]:
        if int(x["where"]) >> 8 >= 6:
            assert int(x["where"]) & 255 == 0 and int(x["problem"]) == 0      # (a pod table only)
            out[int(x["where"]) >> 8][int(x["index"])] = int(x["flags"])
    return out


def mixed_batch(S):
    """A problem whose pods relax, one in which nothing relaxes, an empty one and the smallest problem whose pods stay unscheduled: solved one by one."""
    import audit_reasons_cases as RC
    import audit_stages_cases as SC
    import audit_topo_cases as TC
    from karpenter_core_amd import workloads as W
    name, args = min(RC.FAMILY, key=lambda f: len(RC.stay_problem(**f[1]).pods))
    flats = [S.FlatProblem(p) for p in (SC.relax_problem(1, True), W.config3(140, 3, 1), TC.plain(pods=0), RC.stay_problem(**args))]
    for f in flats:
        f.solve(decode=False)
    return flats


def mixed_batch_both_ways(S):
    """The mixed batch forward and reversed through the wide gate against the eight calls; then what the issue is about: the words of the problems in which nothing
    relaxes -- totals and findings of the seventh pass -- are what each says ALONE (its own call's early-out), whatever its neighbours do.  Returns a summary."""
    flats = mixed_batch(S)
    try:
        eight, g = gate_against_calls(S, flats)
        back, gb = gate_against_calls(S, flats[::-1], masks=(None, ["stages"]))
        relaxing = [d["checked"]["STAGES"] for d in g["passes"]["stages"]]
        assert relaxing[0] > 0 and relaxing[1] == 0 and relaxing[2] == 0, relaxing
        for i, f in enumerate(flats):
            one = S.audit_gate([f], ["stages"], 4096)
            same_totals(S, one, eight_calls(S, [f], passes=["stages"]))      # (alone, the pass's own call leaves early where nothing relaxed)
            alone, j = one["passes"]["stages"][0], len(flats) - 1 - i
            assert alone == g["passes"]["stages"][i] == gb["passes"]["stages"][j], (i, alone, g["passes"]["stages"][i], gb["passes"]["stages"][j])
            rows = lambda x, at: [(int(r["index"]), int(r["flags"])) for r in x["findings"] if r["where"] == 6 << 8 and r["problem"] == at]
            assert rows(one, 0) == rows(g, i) == rows(gb, j), i
        return {"sizes": [f.dims["P"] for f in flats], "stages": relaxing, "clean": g["clean"], "unscheduled": [d["n_unscheduled"] for d in g["passes"]["reasons"]]}
    finally:
        for f in flats:
            f.close()


def silent_edits(S):
    """The four SILENT edits of the stages matrix and the nine edits of the reasons matrix: the six-pass gate is clean on each, the wide gate lists exactly the passes'
    own flagged pods, under pass 6 or 7, and is not clean.  Returns [(name, pass, pods listed)]."""
    import audit_reasons_cases as RC
    import audit_stages_cases as SC
    import audit_stages_ref as SR
    out = []
    flat = S.FlatProblem(SC.tamper_problem())
    flat.solve(decode=False)
    try:
        res, seq, prob = flat.result_arrays(), flat.pod_seq(), SR.problem_arrays(S, flat)
        for name, claimed, s, want in SC.tampers(res, seq, prob):
            if name not in SC.SILENT:
                continue
            old = flat.audit_gate(claimed, s)
            g = flat.audit_gate(claimed, s, passes=list(S.AUDIT_GATE_ALL))
            got = new_pass_findings(g)
            assert old["clean"] and old["n_findings"] == 0, (name, old["n_findings"])
            assert got[6] == want and not g["clean"] and g["passes"]["stages"]["n_pods_flagged"] == len(want), (name, got, want)
            assert got[7] == G_flagged(S._audit("reasons", [flat], claimed)[0]), name      # (whatever the eighth pass makes of an edit to the stages: its own call's rows)
            assert g["n_findings"] == len(got[6]) + len(got[7]), (name, g["n_findings"], got)
            out.append((name, 6, sorted(got[6])))
    finally:
        flat.close()
    pr = RC.tamper_problem()
    flat = S.FlatProblem(pr)
    flat.solve(decode=False)
    try:
        res, seq = flat.result_arrays(), np.array(flat.pod_seq(), dtype=np.int32)
        for name, claimed, want in RC.tampers(res, [p.uid for p in pr.pods]):
            old = flat.audit_gate(claimed, seq)
            g = flat.audit_gate(claimed, seq, passes=list(S.AUDIT_GATE_ALL))
            got = new_pass_findings(g)
            assert old["clean"] and old["n_findings"] == 0, (name, old["n_findings"])
            assert got[7] == want and got[6] == {} and not g["clean"] and g["n_findings"] == len(want), (name, got, want)
            out.append((name, 7, sorted(got[7])))
    finally:
        flat.close()
    return out


def G_flagged(d):
    return {int(i): int(d["pod_flags"][i]) for i in np.nonzero(d["pod_flags"])[0]}


def tail_shapes(S):
    """The shapes at which the tail behind the two passes can go wrong, each through the wide gate against the eight calls: P = 1; P = 257, one row past a 256-row tile
    of the reduction; no pod relaxed at all (the seventh pass's own call leaves after two launches); M = 9 templates for the reasons.  Returns [(name, P)]."""
    import audit_reasons_cases as RC
    import audit_stages_cases as SC
    import audit_topo_cases as TC
    from karpenter_core_amd import fake
    from karpenter_core_amd.model import LABEL_ZONE
    shapes = [("P = 1", SC._open(fake.instance_types(4), [TC._pod("p0", preferred_affinity=SC._prefer((5, LABEL_ZONE, SC.NOWHERE)))])),
              ("P = 257", SC.many_relaxed(257)), ("no pod relaxed at all", TC.plain(3, True)), ("M = 9", RC.stay_problem(**RC.FAMILY[3][1]))]
    out = []
    for name, pr in shapes:
        flat = S.FlatProblem(pr)
        flat.solve(decode=False)
        try:
            eight, g = gate_against_calls(S, [flat], masks=(None, ["stages"], ["reasons"]))
            res, seq = flat.result_arrays(), np.array(flat.pod_seq(), dtype=np.int32)
            claimed = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in res.items() if k != "key_value"}
            claimed["pod_stage"][flat.dims["P"] - 1] += 1      # the last pod claimed one stage on: a finding, or a stage past the chain, in the table's last row
            gate_against_calls(S, [flat], claimed, seq, masks=(None, ["audit", "stages", "reasons"]))
            if name == "no pod relaxed at all":
                assert g["passes"]["stages"][0]["checked"] == {"SEQ": 3, "PODS": 0, "STAGES": 0, "PAIRS": 0}, g["passes"]["stages"][0]
            if name == "M = 9":
                assert flat.dims["M"] == 9 and g["passes"]["reasons"][0]["checked"]["PODS"] > 0, (flat.dims, g["passes"]["reasons"][0])
            out.append((name, flat.dims["P"]))
        finally:
            flat.close()
    return out


def cap_inside_pass_six(S):
    """A findings cap that ends inside pass 6's records: the stages tamper problem with two pods claimed one stage on (pass 6 flags both) and a word on a placed pod
    (pass 7 flags it).  With room for one record: n_findings is still the whole count, pass 7's included, the truncation bit is set, and the table beyond the cap stays
    poisoned.  Returns (n_findings, the records under pass 6, under pass 7)."""
    import audit_stages_cases as SC
    flat = S.FlatProblem(SC.tamper_problem())
    flat.solve(decode=False)
    try:
        res, seq = flat.result_arrays(), np.array(flat.pod_seq(), dtype=np.int32)
        pod = SC.check_genuine(res, seq)
        claimed = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in res.items() if k != "key_value"}
        claimed["pod_stage"][pod["team_a"]] = 1
        claimed["pod_stage"][pod["zonal_a"]] = 1
        claimed["pod_reason"] = np.array(claimed["pod_reason"], dtype=np.uint32)
        claimed["pod_reason"][pod["plain_a"]] = 0x7
        names = ["stages", "reasons"]
        want = expected_findings(S, eight_calls(S, [flat], claimed, seq, names))
        n6, n7 = int((want["where"] >> 8 == 6).sum()), int((want["where"] >> 8 == 7).sum())
        assert n6 == 2 and n7 >= 1, want
        for cap in (1, n6, len(want)):
            table = np.zeros(len(want) + 4, dtype=S.AUDIT_FINDING)
            table.view(np.uint32)[:] = POISON
            g = flat.audit_gate(claimed, seq, passes=names, cap_findings=cap, findings_table=table)
            assert g["n_findings"] == len(want) and g["truncated"] == (cap < len(want)) and not g["clean"], (cap, g["n_findings"], g["truncated"])
            assert table[:cap].tobytes() == want[:cap].tobytes() and (table.view(np.uint32)[4 * cap:] == POISON).all(), (cap, table[:4], want[:4])
        return len(want), n6, n7
    finally:
        flat.close()
