"""A literal Python restatement of the audit's third pass (include/ksolve.h KS_AUDIT_POD_SPREAD, ks_audit_spread_dev): topology spread over narrow keys -- the zone --
decided from the final state and the commit numbers.  One loop per group over the pods in commit order, over the flat problem's arrays and a result in
`FlatProblem.result_arrays()`' form plus `pod_seq`.  No kernel and no library function of the audit's: the rule restates nextDomainTopologySpread's skew inequality
(topologygroup.go:159-200) between a lower bound of the chosen domain's count and an upper bound of the minimum, under the two monotonicities of DESIGN.md 7.22.

    prob = problem_arrays(S, flat)          # audit_topo_ref's: S the scheduler module (the HIP libraries' or the emulator's), flat a FlatProblem
    flags, checked, exact_pairs, skipped_groups = audit(prob, flat.result_arrays(), pod_seq)      # pod_seq: int32 [P] by the problem's own pod indices
"""
import numpy as np

import audit_ref as A
import audit_topo_ref as TR

BITS = {"SEQ": 128, "SPREAD": 2048}
RULES = ("SEQ", "SPREAD")
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
NEVER = 1 << 40

problem_arrays = TR.problem_arrays


def audit(prob: dict, res: dict, pod_seq):
    """(flags uint32 [P], checked [2], exact_pairs, skipped_groups) of result `res` with commit numbers `pod_seq` against problem `prob`."""
    P, E, K, M, G = (prob[k] for k in ("P", "E", "K", "M", "G"))
    N = int(res["n_new"])
    NS = E + N
    pod_node, pod_stage, seq = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(pod_seq, dtype=np.int64)
    flags, checked, exact_pairs = np.zeros(P, dtype=np.uint32), [0, 0], 0
    nstages = lambda p: int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
    cls_of = lambda p: int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + (int(pod_stage[p]) if 0 <= pod_stage[p] < nstages(p) else 0)])
    lst = lambda name, c: [int(x) for x in prob[name[0]][int(prob[name[1]][c]):int(prob[name[1]][c + 1])]]
    own = lambda c: [(x & 0x7FFFFFFF, x >> 31) for x in lst(("own_list", "cls_own_off"), c)]
    sel = lambda c: lst(("sel_list", "cls_sel_off"), c)
    key, typ = (lambda g: int(prob["grp_key"][g])), (lambda g: int(prob["grp_type"][g]))
    skipped = lambda g: not prob["grp_active"][g] or (key(g) >= 0 and int(prob["grp_count"][g * 64]) == INT32_MIN)
    terms = lambda g: range(int(prob["grp_filter_off"][g]), int(prob["grp_filter_off"][g + 1]))
    unfiltered = lambda g: not len(terms(g)) or any(int(prob["flt.present"][f]) == 0 and int(prob["flt.it_state"][f]) == 0 for f in terms(g))
    eligible = [g for g in range(G) if typ(g) == 0 and 0 <= key(g) < K and not skipped(g) and unfiltered(g)]
    skipped_groups = sum(1 for g in range(G) if typ(g) == 0 and g not in eligible)

    # ---- SEQ, by the second pass's definition: a pod that fails it is unplaced below
    placed = [p for p in range(P) if 0 <= pod_node[p] < NS]
    times = {}
    for p in placed:
        times[int(seq[p])] = times.get(int(seq[p]), 0) + 1
    ordered = []
    for p in placed:
        checked[0] += 1
        if 0 <= seq[p] < len(placed) and times[int(seq[p])] == 1:
            ordered.append(p)
        else:
            flags[p] |= BITS["SEQ"]
    ordered.sort(key=lambda p: int(seq[p]))

    def node_req(nd, k):
        return A._req(prob, "en", nd, k) if nd < E else A._node_req(res, K, nd - E, k)

    def fd(nd, k):
        """the node's final In-set on k, or None"""
        r = node_req(nd, k)
        return r.mask if r.present and not r.complement else None

    def one_value(fam, i, k):
        r = A._req(prob, fam, i, k)
        return r.present and not r.complement and bin(r.mask).count("1") == 1

    # ---- pin[n][k]: the least commit number over the pods on n whose class makes the node's requirement on k a single value from that commit on
    pin = {}
    for p in ordered:
        c, nd = cls_of(p), int(pod_node[p])
        for k in range(K):
            if one_value("cls", c, k) or any(typ(g) == 0 and key(g) == k for g, _ in own(c)):
                pin[(nd, k)] = min(pin.get((nd, k), NEVER), int(seq[p]))

    def certain(q, k):
        nd = int(pod_node[q])
        if nd < E:
            r = A._req(prob, "en", nd, k)
            if r.present and not r.complement:
                return True
        else:
            m = int(res["node_tmpl"][nd - E])
            if 0 <= m < M and one_value("tmpl", m, k):
                return True
        return pin.get((nd, k), NEVER) <= int(seq[q])

    def wild(q, k):
        nd = int(pod_node[q])
        return nd < E and not A._req(prob, "en", nd, k).present

    for g in eligible:
        k = key(g)
        init = [int(x) for x in prob["grp_count"][g * 64:(g + 1) * 64]]
        L, U, W = [max(0, x) for x in init], [max(0, x) for x in init], 0
        skew = int(prob["grp_max_skew"][g])
        for p in ordered:      # in commit order: the counts are those of the commits before p's
            c, nd = cls_of(p), int(pod_node[p])
            for gg, self_sel in own(c):
                if gg != g:
                    continue
                mine = fd(nd, k)
                if mine is None:
                    if nd < E and (prob["wellknown_mask"] >> k) & 1 and not node_req(nd, k).present:
                        continue      # 7.22's exception: such a node is Compatible with any requirement on k
                    checked[1] += 1
                    flags[p] |= BITS["SPREAD"]
                    continue
                checked[1] += 1
                if bin(mine).count("1") != 1:
                    flags[p] |= BITS["SPREAD"]
                    continue
                d = mine.bit_length() - 1
                if init[d] < 0:
                    flags[p] |= BITS["SPREAD"]
                    continue
                r = A._req(prob, "cls", c, k)
                has = A.has_mask(r, prob["value_int"][k * 64:(k + 1) * 64], int(prob["key_nvalues"][k])) if r.present else A.ALL
                among = [e for e in range(64) if init[e] >= 0 and (has >> e) & 1]
                least = min([U[e] + W for e in among], default=INT32_MAX)
                if L[d] + self_sel - least > skew:
                    flags[p] |= BITS["SPREAD"]
                if W == 0 and all(L[e] == U[e] for e in among + [d]):
                    exact_pairs += 1
            if g in sel(c):
                theirs = fd(nd, k)
                if theirs is not None and bin(theirs).count("1") == 1:
                    e = theirs.bit_length() - 1
                    U[e] += 1
                    if certain(p, k):
                        L[e] += 1
                elif wild(p, k):
                    W += 1
    return flags, checked, exact_pairs, skipped_groups
