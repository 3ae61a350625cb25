"""A literal Python statement of the audit's eighth pass (include/ksolve.h KS_AUDIT_POD_REASON_*, ks_audit_reasons_dev): the failure reasons.  pod_reason holds,
per unscheduled pod, four bits per machine template: the KS_WHY_* step at which the last scheduler.add refused the pod on a FRESH node of that template.  A fresh
node is static data and Node.Add (node.go:62-107) runs its steps in a fixed order -- taints, host ports, Compatible, topology, topology requirements, instance
types -- so the flat problem alone decides the step for every (class, template) pair no topology group speaks about.  One loop per used class and template over the
flat problem's arrays; no kernel and no library function of the audit's.  The requirement algebra is tests/audit_ref.py's, restated from the reference's Go
(requirement.go, requirements.go), not csrc/ks_algebra.h; the type question is put in tests/audit_firstfit_ref.py's words (compatible && fits && hasOffering).

    prob = problem_arrays(S, flat)
    out = audit(prob, flat.result_arrays())      # a dict: pod_flags, checked [4], the counters, and `decided`: what the exactness test compares with the oracle
`prob["removed"]` (optional): the existing nodes that left the cluster in a what-if -- what a derived view's en_removed says.
"""
import numpy as np

import audit_firstfit_ref as FR
import audit_ref as A

BITS = {"REASON_PLACED": 4194304, "REASON_MISSING": 8388608, "REASON_SHAPE": 16777216, "REASON_STATIC": 33554432}
CHECKED = ("PODS", "EXACT", "BOUNDED", "UNEXAMINED")
WHY = {"NONE": 0, "LIMITS": 1, "TAINTS": 2, "HOST_PORTS": 3, "REQUIREMENTS": 4, "TOPOLOGY": 5, "TOPOLOGY_REQS": 6, "NO_INSTANCE_TYPE": 7}
UNDECIDED, NO_TYPES = "U", "no types"      # s(c, m) beyond the KS_WHY_* values: topology speaks next | the template lists no instance type
UNLIMITED = 0xFFFFFFFF

problem_arrays = FR.problem_arrays


def static_verdict(prob: dict, c: int, m: int):
    """s(c, m): what a fresh node of template m answers class c, in Node.Add's order -- 2, 4, UNDECIDED, 0 or 7; NO_TYPES for a template that lists no type."""
    K, R, T, S, SC = (prob[k] for k in ("K", "R", "T", "S", "SC"))
    TW = (T + 63) // 64
    vi = lambda k: prob["value_int"][k * 64:(k + 1) * 64]
    nv = lambda k: int(prob["key_nvalues"][k])
    wk = lambda k: (prob["wellknown_mask"] >> k) & 1
    count = lambda name: int(prob[name][c + 1]) - int(prob[name][c])
    types = 0
    for w in range(TW):
        types |= int(prob["tmpl_types"][m * TW + w]) << (64 * w)
    if not types:
        return NO_TYPES
    if int(prob["tmpl_taints"][m]) & ~int(prob["cls_tolerated"][c]) & A.ALL:      # Taints.Tolerates, node.go:64
        return WHY["TAINTS"]
    # (HostPortUsage.Validate, node.go:69: a fresh node has no port in use)
    if int(prob["cls_hn_mode"][c]) == 1:      # a fresh node's hostname is a placeholder no pod names, node.go:46
        return WHY["REQUIREMENTS"]
    treq, creq = [A._req(prob, "tmpl", m, k) for k in range(K)], [A._req(prob, "cls", c, k) for k in range(K)]
    if any(A.compatible_fail(treq[k], creq[k], wk(k), vi(k), nv(k)) for k in range(K)):      # nodeRequirements.Compatible(podRequirements), node.go:77: EXACT
        return WHY["REQUIREMENTS"]
    sa, sb = int(prob["tmpl.it_state"][m]), int(prob["cls.it_state"][c])
    if not 0 <= sa < S:
        return WHY["REQUIREMENTS"]
    si = sa
    if SC:
        if not 0 <= sb < SC or prob["its_fail"][sa * SC + sb]:
            return WHY["REQUIREMENTS"]
        si = int(prob["its_inter"][sa * SC + sb])
    if count("cls_own_off") or count("cls_isel_off") or count("cls_port_off"):      # not examinable in the fourth pass's sense: Topology.AddRequirements speaks next
        return UNDECIDED
    if si >= S:
        return WHY["NO_INSTANCE_TYPE"]
    # filterInstanceTypesByRequirements (node.go:137-159) over the template's FULL type set: compatible && fits && hasOffering
    merged = [FR._meet(treq[k], creq[k], vi(k), nv(k)) for k in range(K)]
    rmask = int(prob["tmpl_daemon_present"][m]) | int(prob["cls_requests_present"][c])
    need = [A._wrap64(int(prob["tmpl_daemon"][m * R + r]) + int(prob["cls_requests"][c * R + r])) for r in range(R)]
    allow_z = allow_c = A.ALL
    kz, kc, n_ct = prob["key_zone"], prob["key_ct"], prob["n_ct"]
    if kz >= 0 and merged[kz].present:
        allow_z = A.has_mask(merged[kz], vi(kz), nv(kz))
    if kc >= 0 and merged[kc].present:
        allow_c = A.has_mask(merged[kc], vi(kc), nv(kc))
    pairs = 0
    for z in range(64):
        if (allow_z >> z) & 1 and z * n_ct < 64:
            pairs |= (allow_c & ((1 << n_ct) - 1)) << (z * n_ct)
    pairs = A.ALL if n_ct == 0 else pairs & A.ALL
    for t in range(T):
        if not (types >> t) & 1 or not (int(prob["its_types"][si * TW + t // 64]) >> (t % 64)) & 1:
            continue
        tr = lambda k: A.Req((int(prob["it_present"][t]) >> k) & 1, (int(prob["it_complement"][t]) >> k) & 1, prob["it_mask"][k * T + t])
        if any(merged[k].present and tr(k).present and A.intersects_fail(tr(k), merged[k], vi(k), nv(k)) for k in range(K)):
            continue
        if any((rmask >> r) & 1 and need[r] > int(prob["it_alloc"][r * T + t]) for r in range(R)):
            continue
        if int(prob["it_offer"][t]) & pairs:
            return WHY["NONE"]
    return WHY["NO_INSTANCE_TYPE"]


def expected(s, limited: bool):
    """What the nibble of an unscheduled pod may be, given s(c, m): (kind, allowed values) -- kind "exact", "bounded" or None (not examined).  On a limited
    template KS_WHY_LIMITS is allowed besides and not examined: the caller's case."""
    if s == NO_TYPES:
        return None, ()
    if s == UNDECIDED:
        return "bounded", (WHY["TOPOLOGY"], WHY["TOPOLOGY_REQS"], WHY["NO_INSTANCE_TYPE"])
    if limited and s == WHY["NONE"]:
        return "exact", (WHY["NO_INSTANCE_TYPE"],)      # the limit only shrinks the type set
    return "exact", (s,)


def audit(prob: dict, res: dict) -> dict:
    P, E, M, C = prob["P"], prob["E"], prob["M"], prob["C"]
    MT = min(M, 8)
    NS = E + int(res["n_new"])
    removed = set(int(e) for e in prob.get("removed", ()))
    pod_node, pod_stage, reason = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(res["pod_reason"], dtype=np.uint32)
    flags, checked = np.zeros(P, dtype=np.uint32), [0, 0, 0, 0]
    limited = [int(prob["tmpl_limit_present"][m]) != UNLIMITED for m in range(M)]
    n_placed = n_unscheduled = 0
    verdicts, decided = {}, []
    for p in range(P):
        nd, w = int(pod_node[p]), int(reason[p])
        if 0 <= nd < NS and nd not in removed:      # names a node of the result: both pack kernels and the oracle clear the word on every successful add
            n_placed += 1
            if w:
                flags[p] |= BITS["REASON_PLACED"]
            continue
        if nd != -1:
            continue
        n_unscheduled += 1
        off, n = int(prob["pod_stage_off"][p]), int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
        if not 0 <= pod_stage[p] < n:
            continue      # the first pass's RANGE
        c = int(prob["stage_cls"][off + int(pod_stage[p])])
        if not c < C:
            continue
        checked[0] += 1
        for m in range(8):
            nb = (w >> (4 * m)) & 15
            if m >= M:
                if nb:
                    flags[p] |= BITS["REASON_SHAPE"]      # a template the problem does not have
                continue
            if (c, m) not in verdicts:
                verdicts[(c, m)] = static_verdict(prob, c, m)
            s = verdicts[(c, m)]
            said = False
            if nb == WHY["NONE"]:
                flags[p] |= BITS["REASON_MISSING"]; said = True      # add returns an error only after every template produced one
            elif nb > 7 or nb == WHY["HOST_PORTS"] or (nb == WHY["LIMITS"] and not limited[m]):
                flags[p] |= BITS["REASON_SHAPE"]; said = True
            kind, allowed = expected(s, limited[m])
            if kind is None or (limited[m] and nb == WHY["LIMITS"]):
                checked[3] += 1
                continue
            checked[1 if kind == "exact" else 2] += 1
            if kind == "exact":
                decided.append((p, m, allowed[0], limited[m]))
            if not said and nb not in allowed:
                flags[p] |= BITS["REASON_STATIC"]
    used = sorted({c for c, _ in verdicts})
    assert len(verdicts) == len(used) * MT
    return {"pod_flags": flags, "checked": checked, "skipped_pods": P - n_placed - checked[0], "n_unscheduled": n_unscheduled, "n_placed": n_placed, "n_new": int(res["n_new"]),
            "used_classes": len(used), "pairs": len(verdicts), "decided": decided, "verdicts": verdicts}
