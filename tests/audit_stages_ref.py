"""A literal Python statement of the audit's seventh pass (include/ksolve.h KS_AUDIT_POD_STAGE_*, ks_audit_stages_dev): relaxation order, decided from the final
state.  Solve relaxes a pod one step per failed add (scheduler.go:118-127): a pod that ended at stage k was tried and refused at every stage j < k.  An existing node
was there at every such moment and only filled up, a fresh node of a template without limits is static data -- so where the FINAL state of an existing node, or such
a fresh node, admits the class of stage j, that add cannot have failed.  And the queue ends only on pods whose chain is used up (queue.go:44-68).

The two clauses are the fourth pass's, and they are not restated here: tests/audit_firstfit_ref.py decides them.  Its `audit` raises FIT_EXISTING / FIT_TEMPLATE on an
UNSCHEDULED pod exactly when some existing node / some unlimited template admits the pod's class.  So this file PUTS THE QUESTION to it: a probe problem that holds the
result's pods on their existing nodes (they fill the nodes; a commit number of -1 keeps them from being examined themselves), no new node at all, and one unscheduled
one-stage pod per distinct class c_j of an examined stage.  The probe pod's two bits are admits_existing / admits_template over every node and template, with that
file's examined-pair condition on labelled keys, its volume exception, its removed nodes and its exclusion of limited templates; its pair counts are this pass's.

    prob = problem_arrays(S, flat)
    out = audit(prob, flat.result_arrays(), pod_seq)      # a dict: pod_flags, checked [4], admitting_pairs, skipped_pods, and what the soundness gate counts
`prob["removed"]` (optional): the existing nodes that left the cluster in a what-if -- what a derived view's en_removed says.
"""
import numpy as np

import audit_firstfit_ref as FR

BITS = {"SEQ": 128, "STAGE_EXISTING": 524288, "STAGE_TEMPLATE": 1048576, "STAGE_UNRELAXED": 2097152}
CHECKED = ("SEQ", "PODS", "STAGES", "PAIRS")
STAGE = BITS["STAGE_EXISTING"] | BITS["STAGE_TEMPLATE"] | BITS["STAGE_UNRELAXED"]

problem_arrays = FR.problem_arrays


def admitting_classes(prob: dict, res: dict, classes):
    """{c: (some existing node's final state admits c, some unlimited template admits c)} for `classes`, the pairs evaluated against existing nodes, against templates,
    and the pairs that admitted -- all by tests/audit_firstfit_ref.py's audit over the probe problem (above)."""
    classes = list(classes)
    P, E, U = prob["P"], prob["E"], len(classes)
    removed = set(int(e) for e in prob.get("removed", ()))
    pod_node = np.asarray(res["pod_node"], dtype=np.int64)
    stays = [0 <= int(nd) < E and int(nd) not in removed for nd in pod_node]      # the pods the result puts on an existing node: they fill it
    probe = dict(prob)
    probe["P"] = P + U
    off = [int(x) for x in prob["pod_stage_off"][:P + 1]]
    probe["pod_stage_off"] = np.array(off + [off[P] + u + 1 for u in range(U)], dtype=np.uint32)
    probe["stage_cls"] = np.concatenate([np.asarray(prob["stage_cls"][:off[P]], dtype=np.uint32), np.array(classes, dtype=np.uint32)])
    pres = dict(res)
    pres["n_new"] = 0
    pres["pod_node"] = np.array([int(pod_node[p]) if stays[p] else -2 for p in range(P)] + [-1] * U, dtype=np.int32)      # -2: on no node of the probe, and not unscheduled either
    pres["pod_stage"] = np.concatenate([np.asarray(res["pod_stage"], dtype=np.int32)[:P], np.zeros(U, dtype=np.int32)])
    flags, checked, admitting, _ = FR.audit(probe, pres, np.full(P + U, -1, dtype=np.int32))
    unlimited = sum(1 for m in range(prob["M"]) if int(prob["tmpl_limit_present"][m]) == FR.UNLIMITED)
    found = {c: (bool(flags[P + u] & FR.BITS["FIT_EXISTING"]), bool(flags[P + u] & FR.BITS["FIT_TEMPLATE"])) for u, c in enumerate(classes)}
    return found, checked[2] - U * unlimited, U * unlimited, admitting


def audit(prob: dict, res: dict, pod_seq) -> dict:
    P, E = prob["P"], prob["E"]
    NS = E + int(res["n_new"])
    removed = set(int(e) for e in prob.get("removed", ()))
    pod_node, pod_stage, seq = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64), np.asarray(pod_seq, dtype=np.int64)
    flags, checked = np.zeros(P, dtype=np.uint32), [0, 0, 0, 0]
    chain = lambda p: [int(c) for c in prob["stage_cls"][int(prob["pod_stage_off"][p]):int(prob["pod_stage_off"][p + 1])]]
    count = lambda name, c: int(prob[name][c + 1]) - int(prob[name][c])
    examinable = lambda c: count("cls_own_off", c) == 0 and count("cls_isel_off", c) == 0 and count("cls_port_off", c) == 0      # the fourth pass's sense

    def where(p):
        nd = int(pod_node[p])
        return nd if 0 <= nd < NS and nd not in removed else -1

    # ---- SEQ, by the second pass's definition: a placed pod that fails it is not examined
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

    # ---- UNRELAXED, and the examined stages: j < k of a pod that does not fail SEQ or is unscheduled, pod_stage in range, c_j examinable
    stages = {}
    for p in range(P):
        ch, k = chain(p), int(pod_stage[p])
        if not 0 <= k < len(ch):
            continue
        if pod_node[p] == -1 and k != len(ch) - 1:
            flags[p] |= BITS["STAGE_UNRELAXED"]
        if p in ordered or pod_node[p] == -1:
            mine = [ch[j] for j in range(k) if examinable(ch[j])]
            if mine:
                stages[p] = mine
    checked[1], checked[2] = len(stages), sum(len(v) for v in stages.values())
    used = sorted({c for v in stages.values() for c in v})
    found, pairs_existing, pairs_template, admitting = admitting_classes(prob, res, used) if used else ({}, 0, 0, 0)
    checked[3] = pairs_existing + pairs_template
    for p, mine in stages.items():
        if any(found[c][0] for c in mine):
            flags[p] |= BITS["STAGE_EXISTING"]
        if any(found[c][1] for c in mine):
            flags[p] |= BITS["STAGE_TEMPLATE"]
    return {"pod_flags": flags, "checked": checked, "admitting_pairs": admitting, "skipped_pods": P - len(stages), "pairs_existing": pairs_existing,
            "pairs_template": pairs_template, "unscheduled_examined": sum(1 for p in stages if pod_node[p] == -1), "used_classes": len(used)}
