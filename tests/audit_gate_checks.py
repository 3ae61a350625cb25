"""What the tests of the audit's gate share (tests/test_audit_gate*.py): the comparison of `scheduler.audit_gate` with the six passes' own calls over the same
results -- the reference here: the calls are unchanged by the gate and pinned against the literal references by their own suites --, and a recorder that puts that
comparison behind every call the passes' cases modules (tests/audit_*_cases.py) make, so that every problem, tamper and shape they hold goes through the gate too.
Every function takes the scheduler module `S` it is to go through (the HIP libraries' or the emulator's)."""
import numpy as np

POISON = 0xA5A5A5A5
SUB_MASKS = (["firstfit"], ["audit", "firstfit", "hostfit"], ["limits"])      # a single pass | first + firstfit + hostfit | limits alone (its early-out where no template is limited)


def pod_order_seq(claimed, n_pods):
    """The commit numbers `ksh_audit_claimed` gives the first pass of a claimed result that comes without any: the placed pods numbered in pod order."""
    seq, k = np.full(n_pods, -1, dtype=np.int32), 0
    for i, nd in enumerate(np.asarray(claimed["pod_node"]).reshape(-1)[:n_pods]):
        if nd != -1:
            seq[i], k = k, k + 1
    return seq


def six_calls(S, flats, claimed=None, pod_seq=None, passes=None):
    """{pass: [one dict per problem]} through the passes' own calls (`scheduler._audit`)."""
    audit = getattr(S, "_audit_unrecorded", S._audit)
    return {w: audit(w, flats, claimed, pod_seq if S._AUDIT_PASSES[w]["seq"] else None) for w in (passes or list(S._AUDIT_PASSES))}


def expected_findings(S, six):
    """The non-zero entries of the passes' flag tables in the gate's order: by pass as _AUDIT_PASSES has them, by problem, pods before nodes, by index."""
    rec = []
    for k, w in enumerate(S._AUDIT_PASSES):
        for i, d in enumerate(six.get(w, [])):
            for t, key in enumerate(("pod_flags", "node_flags")):
                if key in d:
                    nz = np.nonzero(d[key])[0]
                    rec += [(i, k << 8 | t, int(x), int(d[key][x])) for x in nz]
    return np.array(rec, dtype=S.AUDIT_FINDING) if rec else np.zeros(0, dtype=S.AUDIT_FINDING)


def same_totals(S, gate, six):
    """Every totals field of every requested pass is what the pass's own call returned: every key of its dict but the flag arrays, the times, and the bit counts the
    binding counts from the rows where the C struct holds none (those are absent from the gate's dict, never different)."""
    assert list(gate["passes"]) == [w for w in S._AUDIT_PASSES if w in six], (list(gate["passes"]), list(six))
    for w, rows in six.items():
        assert len(gate["passes"][w]) == len(rows), w
        for i, (g, d) in enumerate(zip(gate["passes"][w], rows)):
            want = {k: v for k, v in d.items() if k not in ("pod_flags", "node_flags", "ms")}
            derived = set(want) - set(g)
            assert derived <= {"pod_bit_count"} and (not derived or not hasattr(S._AUDIT_PASSES[w]["Out"](), "pod_bit_count")), (w, derived)
            for k in derived:
                del want[k]
            assert g == want, (w, i, {k: (g.get(k), want.get(k)) for k in set(g) | set(want) if g.get(k) != want.get(k)})


def gate_against_calls(S, flats, claimed=None, pod_seq=None, masks=(None,) + SUB_MASKS, cap=4096):
    """The gate over `flats` (or `claimed` for flats[0]) against the six calls: totals, findings, `clean`, twice with equal bytes -- for all six passes and for each
    sub-mask.  Returns (the six calls' dicts, the gate's dict with all six passes)."""
    if claimed is not None and pod_seq is None:
        pod_seq = pod_order_seq(claimed, flats[0].dims["P"])
    six = six_calls(S, flats, claimed, pod_seq)
    full = None
    for names in masks:
        part = six if names is None else {w: six[w] for w in S._AUDIT_PASSES if w in names}
        runs = [S.audit_gate(flats, names, cap, claimed, pod_seq) for _ in range(2)]
        g = runs[0]
        same_totals(S, g, part)
        want = expected_findings(S, part)
        assert g["n_findings"] == len(want) and not g["truncated"], (names, g["n_findings"], len(want), g["truncated"])
        assert g["findings"].tobytes() == want.tobytes(), (names, g["findings"][:8], want[:8])
        assert g["clean"] == (len(want) == 0) == all(not d[k].any() for rows in part.values() for d in rows for k in ("pod_flags", "node_flags") if k in d)
        assert runs[1]["findings"].tobytes() == g["findings"].tobytes() and runs[1]["passes"] == g["passes"] and runs[1]["n_findings"] == g["n_findings"], names
        if names is None:
            full = g
    return six, full


class Recorder:
    """Puts `gate_against_calls` behind every call of a pass that goes through `S._audit` -- the methods of FlatProblem and the batch functions, which is how the cases
    modules audit.  `seen`: [(pass, problems, claimed?, findings)], `gates`: the gate's dict of each; a call the pass refuses raises before the gate is asked."""

    def __init__(self, S, masks=(None,)):
        self.S, self.masks, self.seen, self.gates, self.busy = S, masks, [], [], False
        S._audit_unrecorded = S._audit
        S._audit = self

    def __call__(self, what, flats, claimed=None, pod_seq=None):
        res = self.S._audit_unrecorded(what, flats, claimed, pod_seq)
        if not self.busy and len(flats):
            self.busy = True
            try:
                six, g = gate_against_calls(self.S, flats, claimed, pod_seq, masks=self.masks)
                self.seen.append((what, len(flats), claimed is not None, g["n_findings"]))
                self.gates.append(g)
            finally:
                self.busy = False
        return res

    def remove(self):
        self.S._audit = self.S._audit_unrecorded
        del self.S._audit_unrecorded


def all_flagged_claim(S, flat):
    """A claimed result in which the first pass flags EVERY pod: the genuine result `flat` holds with every pod_stage past the pod's chain (KS_AUDIT_POD_RANGE)."""
    r = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in flat.result_arrays().items() if k != "key_value"}
    r["pod_stage"] = np.full(flat.dims["P"], 1 << 20, dtype=np.int32)
    return r, np.array(flat.pod_seq(), dtype=np.int32)


def findings_at_the_cap(S, flat, claimed, pod_seq):
    """Caps 0, 1, n - 1, n, n + 1 over a claimed result whose n findings of the first pass span several workgroups: n_findings is n in all five, the truncation bit is
    set exactly for the first three, the records are the first min(cap, n) of the full list, and the poisoned table beyond them is untouched."""
    six = six_calls(S, [flat], claimed, pod_seq, ["audit"])
    want = expected_findings(S, six)
    n = len(want)
    assert n >= 600 and six["audit"][0]["n_pods_flagged"] == flat.dims["P"], (n, six["audit"][0]["n_pods_flagged"])
    out = []
    for cap in (0, 1, n - 1, n, n + 1):
        table = np.zeros(n + 8, dtype=S.AUDIT_FINDING)
        table.view(np.uint32)[:] = POISON
        g = flat.audit_gate(claimed, pod_seq, passes=["audit"], cap_findings=cap, findings_table=table)
        m = min(cap, n)
        assert g["n_findings"] == n and g["truncated"] == (cap < n) and not g["clean"], (cap, g["n_findings"], g["truncated"])
        assert len(g["findings"]) == m and table[:m].tobytes() == want[:m].tobytes(), (cap, table[:4], want[:4])
        assert (table.view(np.uint32)[4 * m:] == POISON).all(), cap
        out.append((cap, g["n_findings"], g["truncated"]))
    return out
