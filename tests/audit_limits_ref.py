"""A literal Python restatement of the audit's fifth pass (include/ksolve.h KS_AUDIT_NODE_LIMIT_*, KS_AUDIT_POD_LIMIT_TEMPLATE, ks_audit_limits_dev): provisioner
limits, decided from the final state and the commit numbers.  Before it opens a machine of a limited provisioner scheduler.add keeps only the instance types whose
Capacity is within the provisioner's remaining resources (filterByRemainingResources, scheduler.go:293-309), and after the opener's Add it takes the MaxResources of
the node's options off them (subtractMax, scheduler.go:273-290).  A node's options only shrink, so the final options bound what was taken from below and the types
an opener could have kept bound it from above: an upper bound U and a lower bound L of the remaining at every opening, per limited template, in opening order.
Written from that text and the rule in ksolve.h, not from the kernels; the requirement algebra is tests/audit_ref.py's.

    prob = problem_arrays(S, flat)
    out = audit(prob, flat.result_arrays(), pod_seq)      # a dict: pod_flags, node_flags, checked [4], limited_templates, skipped_nodes, skipped_pods, exact_nodes, binding_nodes
"""
import numpy as np

import audit_ref as A
import audit_topo_ref as TR

POD_BITS = {"SEQ": 128, "LIMIT_TEMPLATE": 32768}
NODE_BITS = {"LIMIT_EXTRA": 256, "LIMIT_MISSING": 512}
CHECKED = ("SEQ", "NODES", "PODS", "PAIRS")
UNLIMITED = 0xFFFFFFFF
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63


def problem_arrays(S, flat) -> dict:
    """audit_topo_ref.problem_arrays plus the tables this pass adds: the lattice's meet, the types' Capacity and the templates' remaining resources."""
    saved = dict(TR.DTYPES)
    try:
        TR.DTYPES.update({"its_inter": np.uint16, "it_cap": np.int64, "tmpl_remaining": np.int64})
        return TR.problem_arrays(S, flat)
    finally:
        TR.DTYPES.clear(); TR.DTYPES.update(saved)


def _meet(a, b, vi, nv):
    if not b.present:
        return a
    if not a.present:
        return b
    return A._intersection(a, b, vi, nv)


def audit(prob: dict, res: dict, pod_seq) -> dict:
    P, E, K, R, T, M, S, SC = (prob[k] for k in ("P", "E", "K", "R", "T", "M", "S", "SC"))
    TW = (T + 63) // 64
    N = int(res["n_new"])
    NS = E + N
    removed = set(int(e) for e in prob.get("removed", ()))
    pod_node, pod_stage, seq = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(pod_seq, dtype=np.int64)
    pod_flags, node_flags, checked = np.zeros(P, dtype=np.uint32), np.zeros(NS, dtype=np.uint32), [0, 0, 0, 0]
    vi = lambda k: prob["value_int"][k * 64:(k + 1) * 64]
    nv = lambda k: int(prob["key_nvalues"][k])
    wk = lambda k: (prob["wellknown_mask"] >> k) & 1
    nstages = lambda p: int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
    cls_of = lambda p: int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + (int(pod_stage[p]) if 0 <= pod_stage[p] < nstages(p) else 0)])
    count = lambda name, c: int(prob[name][c + 1]) - int(prob[name][c])
    examinable = lambda c: count("cls_own_off", c) == 0 and count("cls_isel_off", c) == 0 and count("cls_port_off", c) == 0
    creq = lambda c, r: int(prob["cls_requests"][c * R + r])
    cap = lambda t, r: int(prob["it_cap"][r * T + t])
    lim_of = lambda m: int(prob["tmpl_limit_present"][m])
    lim_res = lambda m: [r for r in range(R) if (lim_of(m) >> r) & 1]
    R0 = lambda m, r: int(prob["tmpl_remaining"][m * R + r])

    def where(p):
        nd = int(pod_node[p])
        return nd if 0 <= nd < NS and nd not in removed else -1

    def bitset(words):
        out = 0
        for w in range(TW):
            out |= int(words[w]) << (64 * w)
        return out & ((1 << T) - 1)
    node_types = lambda j: bitset(np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, TW)[j]) if TW else 0
    tmpl_types = lambda m: bitset(prob["tmpl_types"][m * TW:(m + 1) * TW])
    members = lambda bits: [t for t in range(T) if (bits >> t) & 1]

    # ---- SEQ, by the second pass's definition
    placed = [p for p in range(P) if where(p) >= 0]
    times = {}
    for p in placed:
        times[int(seq[p])] = times.get(int(seq[p]), 0) + 1
    ordered = set()
    for p in placed:
        checked[0] += 1
        if 0 <= seq[p] < len(placed) and times[int(seq[p])] == 1:
            ordered.add(p)
        else:
            pod_flags[p] |= POD_BITS["SEQ"]
    out = {"pod_flags": pod_flags, "node_flags": node_flags, "checked": checked, "limited_templates": 0, "skipped_nodes": 0, "skipped_pods": 0, "exact_nodes": 0,
           "binding_nodes": 0, "n_new": N, "n_placed": len(placed)}
    limited = [m for m in range(M) if lim_of(m) != UNLIMITED]
    out["limited_templates"] = len(limited)
    if not limited:      # nothing of this pass's to examine
        return out

    # ---- open(j) and its opener
    opened, opener = {}, {}
    for p in ordered:
        nd = where(p)
        if nd >= E and (nd - E not in opened or int(seq[p]) < opened[nd - E]):
            opened[nd - E], opener[nd - E] = int(seq[p]), p

    # ---- the type tests: filterInstanceTypesByRequirements (node.go:137-159) per type
    type_req = {}

    def treq(t, k):
        if (t, k) not in type_req:
            type_req[(t, k)] = A.Req((int(prob["it_present"][t]) >> k) & 1, (int(prob["it_complement"][t]) >> k) & 1, prob["it_mask"][k * T + t])
        return type_req[(t, k)]

    def passing(merged, need, rmask, live):
        """the types of `live` that pass compatible && fits && hasOffering against requirements merged[k] and requests need[r] under rmask"""
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
        ok = 0
        for t in members(live):
            if any(merged[k].present and treq(t, k).present and A.intersects_fail(treq(t, k), merged[k], vi(k), nv(k)) for k in range(K)):
                continue
            if any((rmask >> r) & 1 and need[r] > int(prob["it_alloc"][r * T + t]) for r in range(R)):
                continue
            if int(prob["it_offer"][t]) & pairs:
                ok |= 1 << t
        return ok

    def its_set(si):
        out = 0
        for w in range(TW):
            out |= int(prob["its_types"][si * TW + w]) << (64 * w)
        return out

    fresh_cache = {}

    def fresh_types(c, m):
        """the types of tmpl_types[m] that pass for a fresh node of template m holding one pod of class c (the fourth pass's per-type test of admits_template); 0 where
        the instance-type lattice has no meet"""
        if (c, m) in fresh_cache:
            return fresh_cache[(c, m)]
        sa, sb = int(prob["tmpl.it_state"][m]), int(prob["cls.it_state"][c])
        si = None
        if 0 <= sa < S:
            if not SC:
                si = sa
            elif 0 <= sb < SC and not prob["its_fail"][sa * SC + sb]:
                si = int(prob["its_inter"][sa * SC + sb])
                si = si if si < S else None
        got = 0
        if si is not None:
            merged = [_meet(A._req(prob, "tmpl", m, k), A._req(prob, "cls", c, k), vi(k), nv(k)) for k in range(K)]
            need = [A._wrap64(int(prob["tmpl_daemon"][m * R + r]) + creq(c, r)) for r in range(R)]
            got = passing(merged, need, int(prob["tmpl_daemon_present"][m]) | int(prob["cls_requests_present"][c]), tmpl_types(m) & its_set(si))
        fresh_cache[(c, m)] = got
        return got

    def scalar_clauses(c, m):
        """admits_template's clauses that look at no instance type (the fourth pass's)"""
        if int(prob["tmpl_taints"][m]) & ~int(prob["cls_tolerated"][c]) & A.ALL:
            return False
        if int(prob["cls_hn_mode"][c]) == 1:
            return False
        for k in range(K):
            a, b = A._req(prob, "tmpl", m, k), A._req(prob, "cls", c, k)
            if b.present:
                if not wk(k) and not A._nidne(b) and not a.present:
                    return False
                if a.present and A._len0(A._intersection(a, b, vi(k), nv(k))):
                    return False
        return True

    def final_types(j, m):
        """the types of tmpl_types[m] that pass the first pass's final-state filter for new node j"""
        its = int(res["node_it_state"][j])
        if not 0 <= its < S:
            return 0
        merged = [A._node_req(res, K, j, k) for k in range(K)]
        need = [int(x) for x in np.asarray(res["node_requests"], dtype=np.int64).reshape(-1, R)[j]] if R else []
        return passing(merged, need, int(res["node_requests_present"][j]), tmpl_types(m) & its_set(its))

    def max_cap(bits, r):
        return max([0] + [cap(t, r) for t in members(bits)])

    def within(t, m, bound):
        return all(cap(t, r) <= bound[r] for r in lim_res(m))

    def minus(m, taken):
        """R0[m] less the saturating sum of `taken` (a list of {r: quantity}), on lim, not below INT64_MIN"""
        out = {}
        for r in lim_res(m):
            s = 0
            for v in taken:
                s = min(I64_MAX, s + v[r])
            out[r] = max(I64_MIN, R0(m, r) - s)
        return out

    # ---- the nodes of every limited template, in opening order
    nodes_of, unordered = {m: [] for m in limited}, {m: [] for m in limited}
    for j in range(N):
        m = int(res["node_tmpl"][j])
        if not 0 <= m < M:
            out["skipped_nodes"] += 1
            continue
        if m not in nodes_of:
            continue
        checked[1] += 1
        if j in opened:
            nodes_of[m].append(j)
        else:
            unordered[m].append(j)
            out["skipped_nodes"] += 1
    L = {}      # L[m][k], k = 0 .. n_m, for the ordered templates
    for m in limited:
        nodes_of[m].sort(key=lambda j: opened[j])
        whole = not unordered[m]
        mcs, mws, exact = [], [], True
        for j in nodes_of[m] + unordered[m]:
            is_ordered = j in opened
            U = minus(m, mcs) if is_ordered else minus(m, [])
            have = node_types(j)
            if any(not within(t, m, U) for t in members(have)):
                node_flags[E + j] |= NODE_BITS["LIMIT_EXTRA"]
            if any(not within(t, m, U) for t in members(tmpl_types(m))):
                out["binding_nodes"] += 1
            if not is_ordered:
                continue
            Lj = minus(m, mws)
            if whole:
                if exact:
                    out["exact_nodes"] += 1
                if any(not (have >> t) & 1 and within(t, m, Lj) for t in members(final_types(j, m))):
                    node_flags[E + j] |= NODE_BITS["LIMIT_MISSING"]
            W = sum(1 << t for t in members(fresh_types(cls_of(opener[j]), m)) if within(t, m, U))
            mc, mw = {r: max_cap(have, r) for r in lim_res(m)}, {r: max_cap(W, r) for r in lim_res(m)}
            if mc != mw:
                exact = False
            mcs.append(mc); mws.append(mw)
        if whole:
            L[m] = [minus(m, mws[:k]) for k in range(len(mws) + 1)]

    # ---- the pods
    examined = [p for p in range(P) if (p in ordered or pod_node[p] == -1) and examinable(cls_of(p))]
    out["skipped_pods"] = P - len(examined)
    checked[2] = len(examined)
    used = sorted({cls_of(p) for p in examined})
    best = {}      # the largest k at which template m, after its first k openings, still admits class c; -1: at none
    for c in used:
        for m in sorted(L):
            checked[3] += 1
            best[(c, m)] = -1
            if scalar_clauses(c, m):
                for k in range(len(L[m])):      # (L falls with k: the first k that refuses ends it)
                    if any(within(t, m, L[m][k]) for t in members(fresh_types(c, m))):
                        best[(c, m)] = k
                    else:
                        break
    for p in examined:
        c = cls_of(p)
        if pod_node[p] == -1:
            if any(best[(c, m)] >= len(L[m]) - 1 for m in L):
                pod_flags[p] |= POD_BITS["LIMIT_TEMPLATE"]
            continue
        nd = where(p)
        if nd < E or opened.get(nd - E) != int(seq[p]):
            continue
        mine = int(res["node_tmpl"][nd - E])
        if not 0 <= mine < M:
            continue
        for m in L:
            if m < mine and best[(c, m)] >= sum(1 for j in nodes_of[m] if opened[j] < int(seq[p])):
                pod_flags[p] |= POD_BITS["LIMIT_TEMPLATE"]
    return out
