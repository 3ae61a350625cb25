"""A literal Python restatement of the audit's second pass (include/ksolve.h KS_AUDIT_POD_SEQ .. KS_AUDIT_POD_HOSTNAME_SPREAD): pod (anti-)affinity and hostname
spread, decided from the final state and the commit numbers.  One loop per rule, over the flat problem's arrays and a result in `FlatProblem.result_arrays()`' form
plus `pod_seq`.  No kernel and no library function of the audit's: each rule restates the reference's Go -- Topology.Record / AddRequirements (topology.go:120-167)
and TopologyGroup.Get / Record / nextDomain* (topologygroup.go:88-243) -- under the two monotonicities the reference guarantees: a group's domain counts only grow,
a node's requirements only narrow.

    prob = problem_arrays(S, flat)          # S: the scheduler module (the HIP libraries' or the emulator's), flat: a FlatProblem
    flags, checked, skipped_groups = audit(prob, flat.result_arrays(), pod_seq)      # pod_seq: int32 [P] by the problem's own pod indices
"""
import numpy as np

import audit_ref as A

BITS = {"SEQ": 128, "ANTI_AFFINITY": 256, "AFFINITY": 512, "HOSTNAME_SPREAD": 1024}
RULES = ("SEQ", "ANTI_AFFINITY", "AFFINITY", "HOSTNAME_SPREAD")
KEY_HOSTNAME = -2
INT32_MIN = -2 ** 31

SCALARS = {"G": 28, "GH": 32}
DTYPES = {"cls_own_off": np.uint32, "own_list": np.uint32, "cls_sel_off": np.uint32, "sel_list": np.uint32, "cls_isel_off": np.uint32, "isel_list": np.uint32,
          "cls_iown_off": np.uint32, "iown_list": np.uint32, "grp_type": np.uint8, "grp_active": np.uint8, "grp_key": np.int32, "grp_max_skew": np.int32, "grp_count": np.int32,
          "grp_hslot": np.int32, "grph_count": np.int32, "grp_filter_off": np.uint32, "flt.present": np.uint32, "flt.it_state": np.int32, "queue": np.uint32}


def problem_arrays(S, flat) -> dict:
    """audit_ref.problem_arrays plus what this pass reads: the classes' group lists and the groups' tables."""
    saved_s, saved_d = dict(A.SCALARS), dict(A.DTYPES)
    try:
        A.SCALARS.update(SCALARS)
        A.DTYPES.update(DTYPES)
        return A.problem_arrays(S, flat)
    finally:
        A.SCALARS.clear(); A.SCALARS.update(saved_s)
        A.DTYPES.clear(); A.DTYPES.update(saved_d)


def audit(prob: dict, res: dict, pod_seq):
    """(flags uint32 [P], checked [4], skipped_groups) of result `res` with commit numbers `pod_seq` against problem `prob`."""
    P, E, K, M, G, GH = (prob[k] for k in ("P", "E", "K", "M", "G", "GH"))
    N = int(res["n_new"])
    NS = E + N
    pod_node, pod_stage, seq = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(pod_seq, dtype=np.int64)
    flags, checked = np.zeros(P, dtype=np.uint32), [0, 0, 0, 0]
    nstages = lambda p: int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
    cls_of = lambda p: int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + (int(pod_stage[p]) if 0 <= pod_stage[p] < nstages(p) else 0)])
    lst = lambda name, c: [int(x) for x in prob[name[0]][int(prob[name[1]][c]):int(prob[name[1]][c + 1])]]
    own = lambda c: [(x & 0x7FFFFFFF, x >> 31) for x in lst(("own_list", "cls_own_off"), c)]
    isel = lambda c: [(x & 0x7FFFFFFF, 0) for x in lst(("isel_list", "cls_isel_off"), c)]
    recorded_by = {}      # class -> the groups a pod of it is recorded by: sel_list (the non-inverse groups that select it) and iown_list (the inverse groups it owns)

    def records(c, g):
        if c not in recorded_by:
            recorded_by[c] = set(lst(("sel_list", "cls_sel_off"), c) + lst(("iown_list", "cls_iown_off"), c))
        return g in recorded_by[c]
    key, typ = (lambda g: int(prob["grp_key"][g])), (lambda g: int(prob["grp_type"][g]))
    # a group created by a later Topology.Update never saw the earlier commits (topology.go:86-117); (the INT32_MIN row: a what-if the group is absent from)
    skipped = lambda g: not prob["grp_active"][g] or (key(g) >= 0 and int(prob["grp_count"][g * 64]) == INT32_MIN)
    skipped_groups = sum(1 for g in range(G) if skipped(g))
    # an empty node filter: no term, or a term that requires nothing -- MakeTopologyNodeFilter of a pod without node selectors -- which every node is Compatible
    # with (topologynodefilter.go:30-70)
    terms = lambda g: range(int(prob["grp_filter_off"][g]), int(prob["grp_filter_off"][g + 1]))
    unfiltered = lambda g: not len(terms(g)) or any(int(prob["flt.present"][f]) == 0 and int(prob["flt.it_state"][f]) == 0 for f in terms(g))

    # ---- SEQ: the commit numbers of the placed pods are pairwise distinct and below their number; a pod that fails this is unplaced for every other rule
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
    klass = {p: cls_of(p) for p in ordered}
    on_node = {}
    for p in ordered:
        on_node.setdefault(int(pod_node[p]), []).append(p)

    def node_req(nd, k):
        if nd < E:
            return A._req(prob, "en", nd, k)
        return A._node_req(res, K, nd - E, k)

    def dom(nd, k):
        """the node's final requirement on k as an In-set, or None: an existing node's label, a new node's mask when the key is present and no complement"""
        r = node_req(nd, k)
        return r.mask if r.present and not r.complement else None

    def has(nd, k):
        """bit d: Requirement.Has(d) on the node's final requirement (requirement.go:171-176); an absent key has every value"""
        r = node_req(nd, k)
        return A.has_mask(r, prob["value_int"][k * 64:(k + 1) * 64], int(prob["key_nvalues"][k])) if r.present else A.ALL

    def concrete(fam, i, k):
        r = A._req(prob, fam, i, k)
        return r.present and not r.complement

    def certain(q, k):
        """the recorder's node was a concrete set on k at the recorder's own commit, whatever happened later"""
        nd, c = int(pod_node[q]), cls_of(q)
        if nd < E and concrete("en", nd, k):
            return True
        if nd >= E and 0 <= int(res["node_tmpl"][nd - E]) < M and concrete("tmpl", int(res["node_tmpl"][nd - E]), k):
            return True
        if concrete("cls", c, k):
            return True
        # a group on k constrains the recorder: Topology.AddRequirements made the node concrete (topology.go:160-164).  An inverse group created later may not have been there
        return any(key(g) == k for g, _ in own(c)) or any(key(g) == k and not skipped(g) for g, _ in isel(c))

    # ---- first[g][d]: the least commit number over the recorders of narrow-key group g that can have counted domain d
    first = {}
    for q in ordered:
        c, nd = cls_of(q), int(pod_node[q])
        for g in lst(("sel_list", "cls_sel_off"), c) + lst(("iown_list", "cls_iown_off"), c):
            k = key(g)
            if k < 0 or typ(g) == 0 or skipped(g):
                continue
            if typ(g) == 2:      # Record(domains.Values()...): only a certain recorder's final set is within what was counted
                bits = dom(nd, k) if certain(q, k) else None
                bits = bits or 0
            else:                # Record only when Len() == 1; whatever it was, the final requirement Has it
                bits = has(nd, k)
            for d in range(64):
                if (bits >> d) & 1:
                    first[(g, d)] = min(first.get((g, d), 1 << 40), int(seq[q]))

    for p in ordered:
        c, nd, f = cls_of(p), int(pod_node[p]), 0
        for g, self_sel in own(c) + isel(c):
            if skipped(g):
                continue
            k, t = key(g), typ(g)
            if k == KEY_HOSTNAME:
                # exact: a node is one domain, always collapsed
                h = int(prob["grp_hslot"][g])
                if not 0 <= h < GH:
                    continue
                init = max(0, int(prob["grph_count"][h * E + nd])) if nd < E else 0
                before = sum(1 for q in on_node[nd] if q != p and seq[q] < seq[p] and records(klass[q], g))
                if t == 2:                                        # nextDomainAntiAffinity: only a domain with count 0
                    checked[1] += 1
                    if init + before > 0:
                        f |= BITS["ANTI_AFFINITY"]
                elif t == 1:                                      # nextDomainAffinity: only a domain with count > 0 -- unless the bootstrap branch ran, which a self-selecting pod may take
                    if self_sel:
                        continue
                    checked[2] += 1
                    if init + before == 0:
                        f |= BITS["AFFINITY"]
                elif unfiltered(g):      # nextDomainTopologySpread with min 0 (domainMinCount); under a filter Counts depends on the time
                    checked[3] += 1
                    if init + before + self_sel > int(prob["grp_max_skew"][g]):
                        f |= BITS["HOSTNAME_SPREAD"]
                continue
            if k < 0 or k >= K or t == 0 or (t == 1 and self_sel):
                continue
            bit, slot = (BITS["ANTI_AFFINITY"], 1) if t == 2 else (BITS["AFFINITY"], 2)
            mine = dom(nd, k)
            if mine is None:
                # the pod's own topology requirement made its node concrete -- but an existing node is known by its labels, and one without a well-known label
                # is Compatible with any requirement on it (requirements.go:123-133)
                if nd < E and (prob["wellknown_mask"] >> k) & 1 and not node_req(nd, k).present:
                    continue
                checked[slot] += 1
                f |= bit
                continue
            checked[slot] += 1
            for d in range(64):
                if not (mine >> d) & 1:
                    continue
                init = int(prob["grp_count"][g * 64 + d])
                earlier = first.get((g, d), 1 << 40) < seq[p]
                if (init > 0 or earlier) if t == 2 else (init <= 0 and not earlier):
                    f |= bit
        flags[p] |= f
    return flags, checked, skipped_groups
