"""A literal Python restatement of the audit's sixth pass (include/ksolve.h KS_AUDIT_POD_HFIT_*, ks_audit_hostfit_dev): the fourth pass's first-fit order for the pods
whose constraining groups are all hostname-keyed anti-affinity or unfiltered hostname spread.  For such a pod Topology.AddRequirements (topology.go:149-167) adds a
requirement on the hostname alone; a node's hostname is one value for its whole life and a group's count on it only grows (topologygroup.go:101-105) -- so a node whose
FINAL counts admit the pod admitted it at every earlier moment, and the fourth pass's argument carries over.  One loop per used class over the existing nodes, the new
nodes and the templates.  No kernel and no library function of the audit's; the requirement algebra is tests/audit_ref.py's, the problem's arrays and the lattice
meet are tests/audit_firstfit_ref.py's, and the three admits_* predicates are that file's, restated here (they are closures of its `audit`) with ok(c, g, n) conjoined.

    prob = problem_arrays(S, flat)
    flags, checked, admitting_pairs, skipped_pods, eligible_groups, skipped_groups = audit(prob, flat.result_arrays(), pod_seq)
`prob["removed"]` (optional): the existing nodes that left the cluster in a what-if -- what a derived view's en_removed says.
"""
import numpy as np

import audit_ref as A
import audit_firstfit_ref as FR

BITS = {"SEQ": 128, "HFIT_EXISTING": 65536, "HFIT_NEW": 131072, "HFIT_TEMPLATE": 262144}
CHECKED = ("SEQ", "PODS", "PAIRS", "TESTS")
UNLIMITED = FR.UNLIMITED
KEY_HOSTNAME = -2
INT32_MIN = -2 ** 31

problem_arrays = FR.problem_arrays


def audit(prob: dict, res: dict, pod_seq):
    """(flags uint32 [P], checked [4], admitting_pairs, skipped_pods, eligible_groups, skipped_groups) of result `res` with commit numbers `pod_seq` against `prob`."""
    P, E, K, R, T, M, S, SC, G, GH = (prob[k] for k in ("P", "E", "K", "R", "T", "M", "S", "SC", "G", "GH"))
    TW = (T + 63) // 64
    N = int(res["n_new"])
    NS = E + N
    removed = set(int(e) for e in prob.get("removed", ()))
    pod_node, pod_stage, seq = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(pod_seq, dtype=np.int64)
    flags, checked = np.zeros(P, dtype=np.uint32), [0, 0, 0, 0]
    vi = lambda k: prob["value_int"][k * 64:(k + 1) * 64]
    nv = lambda k: int(prob["key_nvalues"][k])
    wk = lambda k: (prob["wellknown_mask"] >> k) & 1
    nstages = lambda p: int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
    cls_of = lambda p: int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + (int(pod_stage[p]) if 0 <= pod_stage[p] < nstages(p) else 0)])
    count = lambda name, c: int(prob[name][c + 1]) - int(prob[name][c])
    lst = lambda name, off, c: [int(x) for x in prob[name][int(prob[off][c]):int(prob[off][c + 1])]]
    creq = lambda c, r: int(prob["cls_requests"][c * R + r])

    # ---- the eligible groups: on the hostname, not skipped (the second pass's definition), anti-affinity or spread with an empty node filter (the second pass's)
    key, typ = (lambda g: int(prob["grp_key"][g])), (lambda g: int(prob["grp_type"][g]))
    skipped = lambda g: not prob["grp_active"][g] or (key(g) >= 0 and int(prob["grp_count"][g * 64]) == INT32_MIN)
    terms = lambda g: range(int(prob["grp_filter_off"][g]), int(prob["grp_filter_off"][g + 1]))
    unfiltered = lambda g: not len(terms(g)) or any(int(prob["flt.present"][f]) == 0 and int(prob["flt.it_state"][f]) == 0 for f in terms(g))
    eligible = set(g for g in range(G) if key(g) == KEY_HOSTNAME and not skipped(g) and 0 <= int(prob["grp_hslot"][g]) < GH and (typ(g) == 2 or (typ(g) == 0 and unfiltered(g))))
    constraining = lambda c: [(x & 0x7FFFFFFF, x >> 31) for x in lst("own_list", "cls_own_off", c)] + [(x & 0x7FFFFFFF, 0) for x in lst("isel_list", "cls_isel_off", c)]
    examinable = lambda c: count("cls_port_off", c) == 0 and len(constraining(c)) > 0 and all(g in eligible for g, _ in constraining(c))

    def where(p):
        nd = int(pod_node[p])
        return nd if 0 <= nd < NS and nd not in removed else -1

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
            flags[p] |= BITS["SEQ"]

    # ---- what the result puts on every node: requests on the existing ones, recorded groups on all (the pods that fail SEQ included), and when every new node opened
    esum, epres, opened, recorded = {}, {}, {}, {}
    for p in placed:
        nd, c = where(p), cls_of(p)
        for g in lst("sel_list", "cls_sel_off", c) + lst("iown_list", "cls_iown_off", c):
            if g in eligible:
                recorded[(g, nd)] = recorded.get((g, nd), 0) + 1
        if nd < E:
            epres[nd] = epres.get(nd, 0) | int(prob["cls_requests_present"][c])
            for r in range(R):
                esum[(nd, r)] = A._wrap64(esum.get((nd, r), 0) + creq(c, r))
        elif p in ordered:
            opened[nd - E] = min(opened.get(nd - E, 1 << 40), int(seq[p]))

    def fin(g, n):
        """init + recorded, or None where the hostname is not registered with the group; n None: a fresh node of a template"""
        if n is None:
            return 0
        init = 0
        if n < E:
            init = -1 if n in removed else int(prob["grph_count"][int(prob["grp_hslot"][g]) * E + n])
        return None if init < 0 else init + recorded.get((g, n), 0)

    def groups_ok(c, n):
        ok = True
        for g, self_sel in constraining(c):      # every test is evaluated
            checked[3] += 1
            v = fin(g, n)
            if typ(g) == 2:      # nextDomainAntiAffinity: registered with count 0
                ok = ok and v == 0
            else:                # nextDomainTopologySpread, the hostname's minimum is 0
                ok = ok and v is not None and v + self_sel <= int(prob["grp_max_skew"][g])
        return ok

    examined = [p for p in range(P) if (p in ordered or pod_node[p] == -1) and examinable(cls_of(p))]
    skipped_pods = P - len(examined)
    checked[1] = len(examined)

    def admits_existing(c, e):
        if int(prob["en_taints"][e]) & ~int(prob["cls_tolerated"][c]) & A.ALL:
            return False
        hm = int(prob["cls_hn_mode"][c])
        if hm:
            inlist = e in [int(x) for x in prob["hn_list"][int(prob["cls_hn_off"][c]):int(prob["cls_hn_off"][c + 1])]]
            if (not inlist) if hm == 1 else inlist:
                return False
        for k in range(K):
            if A.compatible_fail(A._req(prob, "en", e, k), A._req(prob, "cls", c, k), wk(k), vi(k), nv(k)):
                return False
        sa, sb = int(prob["en.it_state"][e]), int(prob["cls.it_state"][c])
        if SC and (not (0 <= sa < S and 0 <= sb < SC) or prob["its_fail"][sa * SC + sb]):
            return False
        rp = int(prob["en_requests_present"][e]) | epres.get(e, 0) | int(prob["cls_requests_present"][c])
        for r in range(R):
            if (rp >> r) & 1 and A._wrap64(int(prob["en_requests"][e * R + r]) + esum.get((e, r), 0) + creq(c, r)) > int(prob["en_avail"][e * R + r]):
                return False
        return True

    type_req = {}

    def treq(t, k):
        if (t, k) not in type_req:
            type_req[(t, k)] = A.Req((int(prob["it_present"][t]) >> k) & 1, (int(prob["it_complement"][t]) >> k) & 1, prob["it_mask"][k * T + t])
        return type_req[(t, k)]

    def admits_node(c, m, nreq, requests, rmask, types, sa):
        if int(prob["tmpl_taints"][m]) & ~int(prob["cls_tolerated"][c]) & A.ALL:
            return False
        if int(prob["cls_hn_mode"][c]) == 1:
            return False
        merged = []
        for k in range(K):
            a, b = nreq(k), A._req(prob, "cls", c, k)
            if b.present:
                if not wk(k) and not A._nidne(b) and not (int(prob["tmpl.present"][m]) >> k) & 1:
                    return False
                if a.present and A._len0(A._intersection(a, b, vi(k), nv(k))):
                    return False
            merged.append(FR._meet(a, b, vi(k), nv(k)))
        sb = int(prob["cls.it_state"][c])
        if not 0 <= sa < S:
            return False
        if SC:
            if not 0 <= sb < SC or prob["its_fail"][sa * SC + sb]:
                return False
            si = int(prob["its_inter"][sa * SC + sb])
            if si >= S:
                return False
        else:
            si = sa
        rmask |= int(prob["cls_requests_present"][c])
        need = [A._wrap64(int(requests[r]) + creq(c, r)) for r in range(R)]
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
        live = types
        for w in range(TW):
            live &= ~(((~int(prob["its_types"][si * TW + w])) & A.ALL) << (64 * w))
        for t in range(T):
            if not (live >> t) & 1:
                continue
            if any(merged[k].present and treq(t, k).present and A.intersects_fail(treq(t, k), merged[k], vi(k), nv(k)) for k in range(K)):
                continue
            if any((rmask >> r) & 1 and need[r] > int(prob["it_alloc"][r * T + t]) for r in range(R)):
                continue
            if int(prob["it_offer"][t]) & pairs:
                return True
        return False

    def bitset(words):
        out = 0
        for w in range(TW):
            out |= int(words[w]) << (64 * w)
        return out

    used = sorted({cls_of(p) for p in examined})
    first, admitting = {}, 0
    for c in used:
        fe = fo = fm = None
        if count("cls_vol_off", c) == 0:
            for e in range(E):
                if e in removed:
                    continue
                if int(prob["cls.present"][c]) & ~int(prob["en.present"][e]) or (int(prob["cls.it_state"][c]) != 0 and int(prob["en.it_state"][e]) == 0):
                    continue
                checked[2] += 1
                if groups_ok(c, e) and admits_existing(c, e):
                    admitting += 1
                    fe = e if fe is None else fe
        for j in range(N):
            m = int(res["node_tmpl"][j])
            if not 0 <= m < M:
                continue
            checked[2] += 1
            req = np.asarray(res["node_requests"], dtype=np.int64).reshape(-1, R)[j] if R else []
            types = bitset(np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, TW)[j]) if TW else 0
            if groups_ok(c, E + j) and admits_node(c, m, lambda k: A._node_req(res, K, j, k), req, int(res["node_requests_present"][j]), types, int(res["node_it_state"][j])):
                admitting += 1
                if j in opened:
                    fo = opened[j] if fo is None else min(fo, opened[j])
        for m in range(M):
            if int(prob["tmpl_limit_present"][m]) != UNLIMITED:
                continue
            checked[2] += 1
            if groups_ok(c, None) and admits_node(c, m, lambda k: A._req(prob, "tmpl", m, k), prob["tmpl_daemon"][m * R:(m + 1) * R], int(prob["tmpl_daemon_present"][m]),
                                                  bitset(prob["tmpl_types"][m * TW:(m + 1) * TW]), int(prob["tmpl.it_state"][m])):
                admitting += 1
                fm = m if fm is None else fm
        first[c] = (fe, fo, fm)

    for p in examined:
        fe, fo, fm = first[cls_of(p)]
        nd = where(p)
        if pod_node[p] == -1:
            if fe is not None:
                flags[p] |= BITS["HFIT_EXISTING"]
            if fo is not None:
                flags[p] |= BITS["HFIT_NEW"]
            if fm is not None:
                flags[p] |= BITS["HFIT_TEMPLATE"]
        elif nd < E:
            if fe is not None and fe < nd:
                flags[p] |= BITS["HFIT_EXISTING"]
        else:
            j = nd - E
            if fe is not None:
                flags[p] |= BITS["HFIT_EXISTING"]
            if opened.get(j) == int(seq[p]):
                if fo is not None and fo < int(seq[p]):
                    flags[p] |= BITS["HFIT_NEW"]
                m = int(res["node_tmpl"][j])
                if 0 <= m < M and fm is not None and fm < m:
                    flags[p] |= BITS["HFIT_TEMPLATE"]
    return flags, checked, admitting, skipped_pods, len(eligible), G - len(eligible)
