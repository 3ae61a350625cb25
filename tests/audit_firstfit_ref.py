"""A literal Python restatement of the audit's fourth pass (include/ksolve.h KS_AUDIT_POD_FIT_*, ks_audit_firstfit_dev): first-fit order, decided from the final state
and the commit numbers.  scheduler.add tries every existing node, then every new node, then every template before it opens a machine (scheduler.go:174-219); a node's
requests only grow, its requirements only narrow, its InstanceTypeOptions only shrink -- so a node whose FINAL state would still take a pod would have taken it at
any earlier moment it existed.  One loop per used class over the existing nodes, the new nodes and the templates, over the flat problem's arrays and a result in
`FlatProblem.result_arrays()`' form plus `pod_seq`.  No kernel and no library function of the audit's; the requirement algebra is tests/audit_ref.py's, restated from
the reference's Go (requirement.go, requirements.go), not csrc/ks_algebra.h.

    prob = problem_arrays(S, flat)          # S: the scheduler module (the HIP libraries' or the emulator's), flat: a FlatProblem
    flags, checked, admitting_pairs, skipped_pods = audit(prob, flat.result_arrays(), pod_seq)      # pod_seq: int32 [P] by the problem's own pod indices
`prob["removed"]` (optional): the existing nodes that left the cluster in a what-if -- what a derived view's en_removed says.
"""
import numpy as np

import audit_ref as A
import audit_topo_ref as TR

BITS = {"SEQ": 128, "FIT_EXISTING": 4096, "FIT_NEW": 8192, "FIT_TEMPLATE": 16384}
CHECKED = ("SEQ", "PODS", "PAIRS")
UNLIMITED = 0xFFFFFFFF


def problem_arrays(S, flat) -> dict:
    """audit_topo_ref.problem_arrays plus the one table this pass adds: the instance-type lattice's meet."""
    saved = dict(TR.DTYPES)
    try:
        TR.DTYPES["its_inter"] = np.uint16
        return TR.problem_arrays(S, flat)
    finally:
        TR.DTYPES.clear(); TR.DTYPES.update(saved)


def _meet(a, b, vi, nv):
    """Requirements.Add on one key (requirements.go:87-94): the side that lacks the key contributes nothing."""
    if not b.present:
        return a
    if not a.present:
        return b
    return A._intersection(a, b, vi, nv)


def audit(prob: dict, res: dict, pod_seq):
    """(flags uint32 [P], checked [3], admitting_pairs, skipped_pods) of result `res` with commit numbers `pod_seq` against problem `prob`."""
    P, E, K, R, T, M, S, SC = (prob[k] for k in ("P", "E", "K", "R", "T", "M", "S", "SC"))
    TW = (T + 63) // 64
    N = int(res["n_new"])
    NS = E + N
    removed = set(int(e) for e in prob.get("removed", ()))
    pod_node, pod_stage, seq = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(pod_seq, dtype=np.int64)
    flags, checked = np.zeros(P, dtype=np.uint32), [0, 0, 0]
    vi = lambda k: prob["value_int"][k * 64:(k + 1) * 64]
    nv = lambda k: int(prob["key_nvalues"][k])
    wk = lambda k: (prob["wellknown_mask"] >> k) & 1
    nstages = lambda p: int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
    cls_of = lambda p: int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + (int(pod_stage[p]) if 0 <= pod_stage[p] < nstages(p) else 0)])
    count = lambda name, c: int(prob[name][c + 1]) - int(prob[name][c])
    examinable = lambda c: count("cls_own_off", c) == 0 and count("cls_isel_off", c) == 0 and count("cls_port_off", c) == 0
    creq = lambda c, r: int(prob["cls_requests"][c * R + r])

    def where(p):
        nd = int(pod_node[p])
        return nd if 0 <= nd < NS and nd not in removed else -1

    # ---- SEQ, by the second pass's definition: a pod that fails it is not examined, and opens nothing
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

    # ---- what the result puts on every existing node (every pod there, whatever its commit number), and when every new node opened
    esum, epres, opened = {}, {}, {}
    for p in placed:
        nd, c = where(p), cls_of(p)
        if nd < E:
            epres[nd] = epres.get(nd, 0) | int(prob["cls_requests_present"][c])
            for r in range(R):
                esum[(nd, r)] = A._wrap64(esum.get((nd, r), 0) + creq(c, r))
        elif p in ordered:
            opened[nd - E] = min(opened.get(nd - E, 1 << 40), int(seq[p]))

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
        for r in range(R):      # resources.Fits: only a resource in the merged list is compared
            if (rp >> r) & 1 and A._wrap64(int(prob["en_requests"][e * R + r]) + esum.get((e, r), 0) + creq(c, r)) > int(prob["en_avail"][e * R + r]):
                return False
        return True

    type_req = {}

    def treq(t, k):
        if (t, k) not in type_req:
            type_req[(t, k)] = A.Req((int(prob["it_present"][t]) >> k) & 1, (int(prob["it_complement"][t]) >> k) & 1, prob["it_mask"][k * T + t])
        return type_req[(t, k)]

    def admits_node(c, m, nreq, requests, rmask, types, sa):
        """admits_new / admits_template: a node of template m whose requirements are nreq(k), whose requests are `requests` under `rmask`, whose options are the bit
        set `types` and whose instance-type state is sa"""
        if int(prob["tmpl_taints"][m]) & ~int(prob["cls_tolerated"][c]) & A.ALL:
            return False
        if int(prob["cls_hn_mode"][c]) == 1:      # a new node's placeholder hostname is in no list (node.go:46)
            return False
        merged = []
        for k in range(K):
            a, b = nreq(k), A._req(prob, "cls", c, k)
            if b.present:
                # "custom labels, if not defined, are denied" at the time (requirements.go:125-130): the template's presence is what every moment of the node had
                if not wk(k) and not A._nidne(b) and not (int(prob["tmpl.present"][m]) >> k) & 1:
                    return False
                # a non-empty intersection, WITHOUT the NotIn / DoesNotExist exception of requirements.go:196-200
                if a.present and A._len0(A._intersection(a, b, vi(k), nv(k))):
                    return False
            merged.append(_meet(a, b, vi(k), nv(k)))
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
        for t in range(T):      # filterInstanceTypesByRequirements, node.go:137-159: compatible && fits && hasOffering
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
        if count("cls_vol_off", c) == 0:      # a class that mounts volumes is examined against new nodes only
            for e in range(E):
                if e in removed:
                    continue
                if int(prob["cls.present"][c]) & ~int(prob["en.present"][e]) or (int(prob["cls.it_state"][c]) != 0 and int(prob["en.it_state"][e]) == 0):
                    continue      # a key the node does not label: the pair is not examined
                checked[2] += 1
                if admits_existing(c, e):
                    admitting += 1
                    fe = e if fe is None else fe
        for j in range(N):
            m = int(res["node_tmpl"][j])
            if not 0 <= m < M:
                continue
            checked[2] += 1
            req = np.asarray(res["node_requests"], dtype=np.int64).reshape(-1, R)[j] if R else []
            types = bitset(np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, TW)[j]) if TW else 0
            if admits_node(c, m, lambda k: A._node_req(res, K, j, k), req, int(res["node_requests_present"][j]), types, int(res["node_it_state"][j])):
                admitting += 1
                if j in opened:
                    fo = opened[j] if fo is None else min(fo, opened[j])
        for m in range(M):
            if int(prob["tmpl_limit_present"][m]) != UNLIMITED:
                continue      # a limited template starts from an order-dependent subset (scheduler.go:199-208)
            checked[2] += 1
            if admits_node(c, m, lambda k: A._req(prob, "tmpl", m, k), prob["tmpl_daemon"][m * R:(m + 1) * R], int(prob["tmpl_daemon_present"][m]),
                           bitset(prob["tmpl_types"][m * TW:(m + 1) * TW]), int(prob["tmpl.it_state"][m])):
                admitting += 1
                fm = m if fm is None else fm
        first[c] = (fe, fo, fm)

    for p in examined:
        fe, fo, fm = first[cls_of(p)]
        nd = where(p)
        if pod_node[p] == -1:
            if fe is not None:
                flags[p] |= BITS["FIT_EXISTING"]
            if fo is not None:
                flags[p] |= BITS["FIT_NEW"]
            if fm is not None:
                flags[p] |= BITS["FIT_TEMPLATE"]
        elif nd < E:
            if fe is not None and fe < nd:
                flags[p] |= BITS["FIT_EXISTING"]
        else:
            j = nd - E
            if fe is not None:
                flags[p] |= BITS["FIT_EXISTING"]
            if opened.get(j) == int(seq[p]):      # the opener; a pod that joined later is checked against existing nodes only
                if fo is not None and fo < int(seq[p]):
                    flags[p] |= BITS["FIT_NEW"]
                m = int(res["node_tmpl"][j])
                if 0 <= m < M and fm is not None and fm < m:
                    flags[p] |= BITS["FIT_TEMPLATE"]
    return flags, checked, admitting, skipped_pods
