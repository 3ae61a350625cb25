"""A literal Python restatement of the audit's ninth pass (include/ksolve.h KS_AUDIT_POD_ZFIT_*, ks_audit_zonefit_dev): first-fit order for the pods whose constraining
groups are all eligible zonal spread groups.  One loop per group over the pods in commit order, in the manner of tests/audit_spread_ref.py, gives every examined pod
the domains that certainly admitted it at its moment s -- the skew inequality of nextDomainTopologySpread (topologygroup.go:155-182) between an UPPER bound of the
domain's count and a LOWER bound of the minimum, the opposite pairing to the third pass's --; then one loop per examined pod over the existing nodes and,
for an opener or an unscheduled pod, over the new nodes opened before s.  No kernel and no library function of the audit's; the requirement algebra is
tests/audit_ref.py's, the problem's arrays and the lattice meet are tests/audit_firstfit_ref.py's, and the two static predicates are that file's, restated here from
the Go (they are closures of its `audit`).

    prob = problem_arrays(S, flat)
    out = audit(prob, flat.result_arrays(), pod_seq)      # {"pod_flags", "checked" [4], "admitting_pairs", "exact_pods", "skipped_pods", "mixed_pods", "eligible_groups", "skipped_groups", "n_new", "n_placed", "pairs_by_kind"}
`prob["removed"]` (optional): the existing nodes that left the cluster in a what-if -- what a derived view's en_removed says.
"""
import numpy as np

import audit_ref as A
import audit_firstfit_ref as FR

BITS = {"SEQ": 128, "ZFIT_EXISTING": 67108864, "ZFIT_NEW": 134217728}
CHECKED = ("SEQ", "PODS", "ZONE", "STATIC")
AZ_GROUPS = 4
KEY_HOSTNAME = -2
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NEVER = 1 << 40

problem_arrays = FR.problem_arrays


def audit(prob: dict, res: dict, pod_seq) -> dict:
    P, E, K, R, T, M, S, SC, G = (prob[k] for k in ("P", "E", "K", "R", "T", "M", "S", "SC", "G"))
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
    own = lambda c: [(x & 0x7FFFFFFF, x >> 31) for x in lst("own_list", "cls_own_off", c)]
    isel = lambda c: [x & 0x7FFFFFFF for x in lst("isel_list", "cls_isel_off", c)]
    sel = lambda c: lst("sel_list", "cls_sel_off", c)

    # ---- the eligible groups: the third pass's definition
    key, typ = (lambda g: int(prob["grp_key"][g])), (lambda g: int(prob["grp_type"][g]))
    skipped = lambda g: not prob["grp_active"][g] or (key(g) >= 0 and int(prob["grp_count"][g * 64]) == INT32_MIN)
    terms = lambda g: range(int(prob["grp_filter_off"][g]), int(prob["grp_filter_off"][g + 1]))
    unfiltered = lambda g: not len(terms(g)) or any(int(prob["flt.present"][f]) == 0 and int(prob["flt.it_state"][f]) == 0 for f in terms(g))
    eligible = set(g for g in range(G) if typ(g) == 0 and 0 <= key(g) < K and not skipped(g) and unfiltered(g))
    examinable = lambda c: count("cls_port_off", c) == 0 and not isel(c) and 1 <= len(own(c)) <= AZ_GROUPS and all(g in eligible for g, _ in own(c))
    mixed = lambda c: any(g in eligible for g, _ in own(c)) and any(g < G and key(g) == KEY_HOSTNAME for g in [g for g, _ in own(c)] + isel(c))

    def where(p):
        nd = int(pod_node[p])
        return nd if 0 <= nd < NS and nd not in removed else -1

    # ---- SEQ, by the second pass's definition
    placed = [p for p in range(P) if where(p) >= 0]
    n_placed = len(placed)
    times = {}
    for p in placed:
        times[int(seq[p])] = times.get(int(seq[p]), 0) + 1
    ordered = []
    for p in placed:
        if 0 <= seq[p] < n_placed and times[int(seq[p])] == 1:
            ordered.append(p)
        else:
            flags[p] |= BITS["SEQ"]
    checked[0] = n_placed
    ordered.sort(key=lambda p: int(seq[p]))
    in_order = set(ordered)

    examined = [p for p in range(P) if (p in in_order or pod_node[p] == -1) and examinable(cls_of(p))]
    is_examined = set(examined)
    checked[1] = len(examined)
    skipped_pods = P - len(examined)
    mixed_pods = sum(1 for p in range(P) if p not in is_examined and mixed(cls_of(p)))

    # ---- what the result puts on the existing nodes (the pods that fail SEQ included), and when every new node opened
    esum, epres, opened = {}, {}, {}
    for p in placed:
        nd, c = where(p), cls_of(p)
        if nd < E:
            epres[nd] = epres.get(nd, 0) | int(prob["cls_requests_present"][c])
            for r in range(R):
                esum[(nd, r)] = A._wrap64(esum.get((nd, r), 0) + creq(c, r))
        elif p in in_order:
            opened[nd - E] = min(opened.get(nd - E, NEVER), int(seq[p]))

    # ---- the third pass's recorders: the node's final In-set, pin[n][k], certain, wild
    def node_req(nd, k):
        return A._req(prob, "en", nd, k) if nd < E else A._node_req(res, K, nd - E, k)

    def fd(nd, k):
        r = node_req(nd, k)
        return r.mask if r.present and not r.complement else None

    def one_value(fam, i, k):
        r = A._req(prob, fam, i, k)
        return r.present and not r.complement and bin(r.mask).count("1") == 1

    pin = {}
    for p in ordered:
        c, nd = cls_of(p), int(pod_node[p])
        for k in range(K):
            if one_value("cls", c, k) or any(typ(g) == 0 and key(g) == k for g, _ in own(c)):
                pin[(nd, k)] = min(pin.get((nd, k), NEVER), int(seq[p]))

    def certain_at(nd, k, sq):
        """was the requirement of node nd on key k one value when the pod with commit number sq was recorded?"""
        if nd < E:
            r = A._req(prob, "en", nd, k)
            if r.present and not r.complement:
                return True
        else:
            m = int(res["node_tmpl"][nd - E])
            if 0 <= m < M and one_value("tmpl", m, k):
                return True
        return pin.get((nd, k), NEVER) <= sq

    # ---- OK_s[g] for every examined pod: one loop per group over the pods in commit order
    okmask, exact = {}, {p: True for p in examined}

    def masks(p, c, g, L, U, W, init, skew):
        k = key(g)
        r = A._req(prob, "cls", c, k)
        has = A.has_mask(r, vi(k), nv(k)) if r.present else A.ALL
        registered = [e for e in range(64) if init[e] >= 0]
        among = [e for e in registered if (has >> e) & 1]
        for i, (gg, self_sel) in enumerate(own(c)):
            if gg != g:
                continue
            if not among:      # Go's MaxInt32 minimum admits everything: nothing is proved from it
                okmask[(p, i)] = 0
                exact[p] = False
                continue
            least = min(L[e] for e in among)
            okmask[(p, i)] = sum(1 << e for e in registered if U[e] + W + self_sel - least <= skew)
            if W != 0 or any(L[e] != U[e] for e in registered):
                exact[p] = False

    for g in sorted(eligible):
        k = key(g)
        init = [int(x) for x in prob["grp_count"][g * 64:(g + 1) * 64]]
        L, U, W = [max(0, x) for x in init], [max(0, x) for x in init], 0
        skew = int(prob["grp_max_skew"][g])
        for p in ordered:      # in commit order: the counts are those of the commits before p's
            c, nd = cls_of(p), int(pod_node[p])
            if p in is_examined:
                masks(p, c, g, L, U, W, init, skew)
            if g in sel(c):
                theirs = fd(nd, k)
                if theirs is not None and bin(theirs).count("1") == 1:
                    e = theirs.bit_length() - 1
                    U[e] += 1
                    if certain_at(nd, k, int(seq[p])):
                        L[e] += 1
                elif nd < E and not A._req(prob, "en", nd, k).present:
                    W += 1
        for p in examined:      # the unscheduled pods were tried last against the final state: the prefix at n_placed
            if pod_node[p] == -1:
                masks(p, cls_of(p), g, L, U, W, init, skew)
    exact_pods = sum(1 for p in examined if exact[p])

    # ---- the fourth pass's static predicates
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

    def admits_new(c, j):
        m = int(res["node_tmpl"][j])
        if int(prob["tmpl_taints"][m]) & ~int(prob["cls_tolerated"][c]) & A.ALL:
            return False
        if int(prob["cls_hn_mode"][c]) == 1:
            return False
        merged = []
        for k in range(K):
            a, b = A._node_req(res, K, j, k), A._req(prob, "cls", c, k)
            if b.present:
                if not wk(k) and not A._nidne(b) and not (int(prob["tmpl.present"][m]) >> k) & 1:
                    return False
                if a.present and A._len0(A._intersection(a, b, vi(k), nv(k))):
                    return False
            merged.append(FR._meet(a, b, vi(k), nv(k)))
        sa, sb = int(res["node_it_state"][j]), int(prob["cls.it_state"][c])
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
        rmask = int(res["node_requests_present"][j]) | int(prob["cls_requests_present"][c])
        requests = np.asarray(res["node_requests"], dtype=np.int64).reshape(-1, R)[j] if R else []
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
        words = np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, TW)[j] if TW else []
        live = 0
        for w in range(TW):
            live |= (int(words[w]) & int(prob["its_types"][si * TW + w])) << (64 * w)
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

    # ---- one loop per examined pod over its targets
    admitting, by_kind = 0, [0, 0]
    for p in examined:
        c, nd = cls_of(p), where(p)
        unsched = pod_node[p] == -1
        s = n_placed if unsched else int(seq[p])
        groups = own(c)
        first_e = first_new = None
        if count("cls_vol_off", c) == 0:      # a class that mounts volumes is examined against new nodes only
            for e in range(E):
                if e in removed:
                    continue
                checked[2] += 1
                by_kind[0] += 1
                zone_ok = True
                for i, (g, _) in enumerate(groups):
                    z = fd(e, key(g))      # an existing node's requirement on a key is its label
                    if z is None or bin(z).count("1") != 1 or not (okmask[(p, i)] >> (z.bit_length() - 1)) & 1:
                        zone_ok = False
                        break
                if not zone_ok:
                    continue
                checked[3] += 1
                if int(prob["cls.present"][c]) & ~int(prob["en.present"][e]) or (int(prob["cls.it_state"][c]) != 0 and int(prob["en.it_state"][e]) == 0):
                    continue      # the fourth pass's condition: every key the class names is labelled on e
                if admits_existing(c, e):
                    admitting += 1
                    if not 0 <= nd < E or e < nd:      # a pod on existing node e_P: only a node before e_P
                        first_e = e if first_e is None else first_e
        opener = unsched or (nd >= E and opened.get(nd - E) == int(seq[p]))
        if opener and s > 0:
            for j in range(N):
                if not 0 <= int(res["node_tmpl"][j]) < M or opened.get(j, NEVER) >= s:
                    continue
                checked[2] += 1
                by_kind[1] += 1
                zone_ok = True
                for i, (g, _) in enumerate(groups):
                    k = key(g)
                    z = fd(E + j, k)
                    if not certain_at(E + j, k, s - 1) or z is None or bin(z).count("1") != 1 or not (okmask[(p, i)] >> (z.bit_length() - 1)) & 1:
                        zone_ok = False
                        break
                if not zone_ok:
                    continue
                checked[3] += 1
                if admits_new(c, j):
                    admitting += 1
                    first_new = opened[j] if first_new is None else min(first_new, opened[j])
        if first_e is not None:
            flags[p] |= BITS["ZFIT_EXISTING"]
        if first_new is not None:
            flags[p] |= BITS["ZFIT_NEW"]
    return {"pod_flags": flags, "checked": checked, "admitting_pairs": admitting, "exact_pods": exact_pods, "skipped_pods": skipped_pods, "mixed_pods": mixed_pods,
            "eligible_groups": len(eligible), "skipped_groups": G - len(eligible), "n_new": N, "n_placed": n_placed,
            "pairs_by_kind": by_kind}      # (existing nodes | new nodes: the reference's own count, which the device does not split)
