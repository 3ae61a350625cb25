"""A literal numpy / Python restatement of the audit (include/ksolve.h KS_AUDIT_*): the checks of `ks_audit_dev`, one loop per table row, over the flat problem's
arrays (`ksh_problem`, walked through `ks_debug_problem_array`) and a result in `FlatProblem.result_arrays()`' form.  No kernel, no library function of the audit's:
the requirement algebra below restates the reference's Go (pkg/scheduling/requirement.go, requirements.go), not csrc/ks_algebra.h.

    prob = problem_arrays(S, flat)          # S: the scheduler module (the HIP libraries' or the emulator's), flat: a FlatProblem
    pod_flags, node_flags = audit(prob, flat.result_arrays())
"""
import ctypes

import numpy as np

POD = {"RANGE": 1, "UNSCHEDULED_LIST": 2, "TAINTS": 4, "REQUIREMENTS": 8, "HOSTNAME": 16, "PORTS": 32, "VOLUME_ERROR": 64}
NODE = {"RESOURCES": 1, "VOLUMES": 2, "EMPTY": 4, "TEMPLATE": 8, "REQUESTS": 16, "OPTIONS_EMPTY": 32, "OPTIONS_EXTRA": 64, "OPTIONS_MISSING": 128}

# the scalar members of ks_problem the audit reads, by byte offset (include/ksolve.h; tests/test_problem_arrays.py checks the struct's layout)
SCALARS = {"P": 0, "C": 4, "T": 8, "M": 12, "E": 16, "K": 20, "R": 24, "S": 36, "SC": 40, "max_new_nodes": 44, "wellknown_mask": 52, "key_zone": 72, "key_ct": 76, "n_ct": 80,
           "ND": 392, "SW": 396}
SIGNED = {"key_zone", "key_ct"}
SIZEOF = 784
DTYPES = {"key_nvalues": np.uint32, "value_int": np.int32, "it_present": np.uint32, "it_complement": np.uint32, "it_mask": np.uint64, "it_offer": np.uint64, "it_alloc": np.int64,
          "its_fail": np.uint8, "its_types": np.uint64, "tmpl_taints": np.uint64, "tmpl_types": np.uint64, "tmpl_daemon": np.int64, "tmpl_daemon_present": np.uint32,
          "tmpl_limit_present": np.uint32, "en_taints": np.uint64, "en_avail": np.int64, "en_requests": np.int64, "en_requests_present": np.uint32, "en_port_off": np.uint32,
          "cls_hn_mode": np.uint8, "cls_hn_off": np.uint32, "hn_list": np.uint32, "cls_requests": np.int64, "cls_requests_present": np.uint32, "cls_tolerated": np.uint64,
          "cls_port_off": np.uint32, "ports": np.uint64, "en_vol_limit": np.int32, "en_vol_count": np.int32, "en_vol_set": np.uint64, "cls_vol_off": np.uint32, "vol_list": np.uint32,
          "pod_stage_off": np.uint32, "stage_cls": np.uint32}
for _f in ("tmpl", "en", "cls"):
    DTYPES.update({_f + ".present": np.uint32, _f + ".complement": np.uint32, _f + ".mask": np.uint64, _f + ".gt": np.int32, _f + ".lt": np.int32, _f + ".it_state": np.int32})


def problem_arrays(S, flat) -> dict:
    """The scalars and arrays of the flat problem behind `flat`, copied: {"P": ..., "it_mask": uint64 array, "cls.mask": ..., ...}."""
    ks, kh = S.libs()
    kh.ksh_problem.restype = ctypes.c_void_p
    kh.ksh_problem.argtypes = [ctypes.c_void_p]
    p = kh.ksh_problem(flat._h)
    raw = ctypes.string_at(p, SIZEOF)
    out = {k: int.from_bytes(raw[o:o + 4], "little", signed=k in SIGNED) for k, o in SCALARS.items()}
    ks.ks_debug_problem_array.restype = ctypes.c_uint32
    ks.ks_debug_problem_array.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    n = ks.ks_debug_problem_array(p, 0xFFFFFFFF, None, None, None, None, None)
    for i in range(n):
        name, eb, cnt, off, marks = ctypes.c_char_p(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        ks.ks_debug_problem_array(p, i, ctypes.byref(name), ctypes.byref(eb), ctypes.byref(cnt), ctypes.byref(off), ctypes.byref(marks))
        nm = name.value.decode()
        if nm not in DTYPES:
            continue
        dt = np.dtype(DTYPES[nm])
        assert dt.itemsize == eb.value, nm
        ptr = int.from_bytes(raw[off.value:off.value + 8], "little")
        out[nm] = np.frombuffer(ctypes.string_at(ptr, cnt.value * eb.value), dtype=dt).copy() if ptr and cnt.value else np.zeros(0, dtype=dt)
    return out


# ---------------------------------------------------------------------------------------------------------------- the requirement algebra, from the Go
NOGT, NOLT, NOT_INT = -2 ** 31, 2 ** 31 - 1, -2 ** 31
ALL = (1 << 64) - 1


class Req:
    """Requirement{complement, values, greaterThan, lessThan} over one key's interned universe (requirement.go:36-42); `present`: the key is in the Requirements."""
    def __init__(self, present, complement, mask, gt=NOGT, lt=NOLT):
        self.present, self.complement, self.mask, self.gt, self.lt = bool(present), bool(complement), int(mask), int(gt), int(lt)


def _within(value_int, nvalues, gt, lt):
    """withinIntPtrs over the universe (requirement.go:227-243)."""
    if gt == NOGT and lt == NOLT:
        return ALL
    w = 0
    for v in range(nvalues):
        x = int(value_int[v])
        if x == NOT_INT or (gt != NOGT and gt >= x) or (lt != NOLT and lt <= x):
            continue
        w |= 1 << v
    return w


def _intersection(a, b, value_int, nvalues):
    """Requirement.Intersection (requirement.go:117-150)."""
    gt, lt = max(a.gt, b.gt), min(a.lt, b.lt)
    if gt != NOGT and lt != NOLT and gt >= lt:
        return Req(True, False, 0)
    if a.complement and b.complement:
        vals = a.mask | b.mask
    elif a.complement:
        vals = b.mask & ~a.mask
    elif b.complement:
        vals = a.mask & ~b.mask
    else:
        vals = a.mask & b.mask
    vals &= _within(value_int, nvalues, gt, lt) & ALL
    comp = a.complement and b.complement
    return Req(True, comp, vals, gt if comp else NOGT, lt if comp else NOLT)


def _len0(r):
    return not r.complement and r.mask == 0


def _nidne(r):
    """Operator() in {NotIn, DoesNotExist} (requirement.go:186-197)."""
    return r.mask != 0 if r.complement else r.mask == 0


def intersects_fail(existing, incoming, value_int, nvalues):
    """Requirements.Intersects on one key (requirements.go:189-206); True == an error."""
    if not existing.present or not incoming.present:
        return False
    if not _len0(_intersection(existing, incoming, value_int, nvalues)):
        return False
    return not (_nidne(incoming) and _nidne(existing))


def compatible_fail(receiver, incoming, well_known, value_int, nvalues):
    """Requirements.Compatible on one key (requirements.go:123-133); True == an error."""
    if not incoming.present:
        return False
    if not well_known and not receiver.present and not _nidne(incoming):
        return True
    return intersects_fail(receiver, incoming, value_int, nvalues)


def has_mask(r, value_int, nvalues):
    """bit v: r.Has(value v) (requirement.go:171-176)."""
    univ = ALL if nvalues >= 64 else (1 << nvalues) - 1
    return ((~r.mask & ALL) if r.complement else r.mask) & univ & _within(value_int, nvalues, r.gt, r.lt)


def _req(prob, fam, i, k):
    K = prob["K"]
    return Req((int(prob[fam + ".present"][i]) >> k) & 1, (int(prob[fam + ".complement"][i]) >> k) & 1, prob[fam + ".mask"][i * K + k], prob[fam + ".gt"][i * K + k], prob[fam + ".lt"][i * K + k])


def _node_req(res, K, j, k):
    gt = res["node_gt"].reshape(-1, K)[j, k] if "node_gt" in res else NOGT
    lt = res["node_lt"].reshape(-1, K)[j, k] if "node_lt" in res else NOLT
    return Req((int(res["node_present"][j]) >> k) & 1, (int(res["node_complement"][j]) >> k) & 1, res["node_mask"].reshape(-1, K)[j, k], gt, lt)


def _port_match(a, b):
    """entry.matches (hostportusage.go:45-57)."""
    a, b = int(a), int(b)
    if a >> 32 != b >> 32:
        return False
    ia, ib = a & 0xFFFFFFFF, b & 0xFFFFFFFF
    return ia == ib or ia == 0 or ib == 0


def _wrap64(x):
    x &= ALL
    return x - (1 << 64) if x >> 63 else x


# ---------------------------------------------------------------------------------------------------------------- the audit
def audit(prob: dict, res: dict):
    """(pod_flags uint32 [P], node_flags uint32 [E + n_new]) of result `res` against problem `prob`."""
    P, E, K, R, T, M, S, SC, ND, SW = (prob[k] for k in ("P", "E", "K", "R", "T", "M", "S", "SC", "ND", "SW"))
    TW = (T + 63) // 64
    N = int(res["n_new"])
    NS = E + N
    pod_node, pod_stage = np.asarray(res["pod_node"], dtype=np.int64), np.asarray(res["pod_stage"], dtype=np.int64)
    pod_seq = np.asarray(res["pod_seq"], dtype=np.int64) if "pod_seq" in res else None
    pf, nf = np.zeros(P, dtype=np.uint32), np.zeros(NS, dtype=np.uint32)
    vi = lambda k: prob["value_int"][k * 64:(k + 1) * 64]
    nv = lambda k: int(prob["key_nvalues"][k])
    nstages = lambda p: int(prob["pod_stage_off"][p + 1]) - int(prob["pod_stage_off"][p])
    stage_ok = lambda p: 0 <= pod_stage[p] < nstages(p)
    cls_of = lambda p: int(prob["stage_cls"][int(prob["pod_stage_off"][p]) + (int(pod_stage[p]) if stage_ok(p) else 0)])      # (a stage outside the chain is flagged; the pod's node counts it at stage 0)
    listed = np.zeros(P, dtype=np.int64)
    for u in np.asarray(res["unscheduled"], dtype=np.int64):
        if 0 <= u < P:
            listed[u] += 1
    on_node = [[] for _ in range(NS)]
    # ---- pods ----
    for p in range(P):
        f, nd = 0, int(pod_node[p])
        in_range = -1 <= nd < NS
        if not in_range or not stage_ok(p):
            f |= POD["RANGE"]
        if pod_seq is not None and (pod_seq[p] != -1 if nd == -1 else pod_seq[p] < 0):
            f |= POD["RANGE"]
        if (listed[p] != 1) if nd == -1 else (listed[p] != 0):
            f |= POD["UNSCHEDULED_LIST"]
        if in_range and nd >= 0:
            on_node[nd].append(p)
        if in_range and nd >= 0 and stage_ok(p):
            c = cls_of(p)
            existing, j = nd < E, nd - E
            m = 0 if existing else int(res["node_tmpl"][j])
            if existing or 0 <= m < M:
                taints = int(prob["en_taints"][nd]) if existing else int(prob["tmpl_taints"][m])
                if taints & ~int(prob["cls_tolerated"][c]) & ALL:
                    f |= POD["TAINTS"]
            bad = False
            for k in range(K):
                b = _req(prob, "cls", c, k)
                if existing:
                    bad |= compatible_fail(_req(prob, "en", nd, k), b, (prob["wellknown_mask"] >> k) & 1, vi(k), nv(k))
                else:
                    bad |= intersects_fail(_node_req(res, K, j, k), b, vi(k), nv(k))
            sa, sb = int(prob["en.it_state"][nd]) if existing else int(res["node_it_state"][j]), int(prob["cls.it_state"][c])
            if SC and (not (0 <= sa < S and 0 <= sb < SC) or prob["its_fail"][sa * SC + sb]):
                bad = True
            if bad:
                f |= POD["REQUIREMENTS"]
            hm = int(prob["cls_hn_mode"][c])
            if hm:
                inlist = existing and nd in [int(x) for x in prob["hn_list"][int(prob["cls_hn_off"][c]):int(prob["cls_hn_off"][c + 1])]]
                if (not inlist) if hm == 1 else inlist:
                    f |= POD["HOSTNAME"]
            if existing and any(int(x) == 0xFFFFFFFF for x in prob["vol_list"][int(prob["cls_vol_off"][c]):int(prob["cls_vol_off"][c + 1])]):
                f |= POD["VOLUME_ERROR"]
        pf[p] = f
    ports_of = lambda c: [int(x) for x in prob["ports"][int(prob["cls_port_off"][c]):int(prob["cls_port_off"][c + 1])]]
    vols_of = lambda c: [int(x) for x in prob["vol_list"][int(prob["cls_vol_off"][c]):int(prob["cls_vol_off"][c + 1])]]
    # ---- nodes ----
    for s in range(NS):
        pods = on_node[s]
        existing, j = s < E, s - E
        if not pods:
            nf[s] = 0 if existing else NODE["EMPTY"]
            continue
        f = 0
        classes = [cls_of(p) for p in pods]
        total = [_wrap64(sum(int(prob["cls_requests"][c * R + r]) for c in classes)) for r in range(R)]
        present = 0
        for c in classes:
            present |= int(prob["cls_requests_present"][c])
        # host ports: every entry of a pod against the node's reservations and every other pod's entries
        for a, (p, c) in enumerate(zip(pods, classes)):
            others = [x for b, c2 in enumerate(classes) if b != a for x in ports_of(c2)]
            if existing:
                others += [int(x) for x in prob["ports"][int(prob["en_port_off"][s]):int(prob["en_port_off"][s + 1])]]
            if any(_port_match(x, y) for x in ports_of(c) for y in others):
                pf[p] |= POD["PORTS"]
        if existing:
            rp = int(prob["en_requests_present"][s]) | present
            if any((rp >> r) & 1 and _wrap64(int(prob["en_requests"][s * R + r]) + total[r]) > int(prob["en_avail"][s * R + r]) for r in range(R)):
                f |= NODE["RESOURCES"]
            drivers = {(e >> 24) & 63 for c in classes for e in vols_of(c) if e != 0xFFFFFFFF}
            for d in sorted(drivers):
                counted = sum(e & 0xFFFFFF for c in classes for e in vols_of(c) if e != 0xFFFFFFFF and e >> 31 and (e >> 24) & 63 == d)
                shared = {e & 0xFFFFFF for c in classes for e in vols_of(c) if not e >> 31 and (e >> 24) & 63 == d}
                fresh = [i for i in shared if not (int(prob["en_vol_set"][s * SW + (i >> 6)]) >> (i & 63)) & 1]
                if int(prob["en_vol_count"][s * ND + d]) + counted + len(fresh) > int(prob["en_vol_limit"][s * ND + d]):
                    f |= NODE["VOLUMES"]
            nf[s] = f
            continue
        m = int(res["node_tmpl"][j])
        if not 0 <= m < M:
            nf[s] = NODE["TEMPLATE"]
            continue
        req = np.asarray(res["node_requests"], dtype=np.int64).reshape(-1, R)[j] if R else []
        rmask = int(res["node_requests_present"][j])
        if rmask != (int(prob["tmpl_daemon_present"][m]) | present) or any(int(req[r]) != _wrap64(int(prob["tmpl_daemon"][m * R + r]) + total[r]) for r in range(R)):
            f |= NODE["REQUESTS"]
        have = 0
        for w in range(TW):
            have |= int(np.asarray(res["node_types"], dtype=np.uint64).reshape(-1, TW)[j, w]) << (64 * w)
        its = int(res["node_it_state"][j])
        allow_z = allow_c = ALL
        kz, kc, n_ct = prob["key_zone"], prob["key_ct"], prob["n_ct"]
        if kz >= 0 and _node_req(res, K, j, kz).present:
            allow_z = has_mask(_node_req(res, K, j, kz), vi(kz), nv(kz))
        if kc >= 0 and _node_req(res, K, j, kc).present:
            allow_c = has_mask(_node_req(res, K, j, kc), vi(kc), nv(kc))
        pairs = 0
        for z in range(64):
            if (allow_z >> z) & 1 and z * n_ct < 64:
                pairs |= (allow_c & ((1 << n_ct) - 1)) << (z * n_ct)
        pairs = ALL if n_ct == 0 else pairs & ALL
        passing = 0
        for t in range(T):
            ok = 0 <= its < S and (int(prob["tmpl_types"][m * TW + t // 64]) >> (t % 64)) & 1 and (int(prob["its_types"][its * TW + t // 64]) >> (t % 64)) & 1
            for k in range(K):
                if not ok:
                    break
                nr = _node_req(res, K, j, k)
                tr = Req((int(prob["it_present"][t]) >> k) & 1, (int(prob["it_complement"][t]) >> k) & 1, prob["it_mask"][k * T + t])
                if nr.present and tr.present and intersects_fail(tr, nr, vi(k), nv(k)):      # instanceType.Requirements.Intersects(nodeRequirements), node.go:143
                    ok = False
            if ok and any((rmask >> r) & 1 and int(req[r]) > int(prob["it_alloc"][r * T + t]) for r in range(R)):      # resources.Fits(requests, Allocatable()), node.go:147
                ok = False
            if ok and not int(prob["it_offer"][t]) & pairs:      # hasOffering, node.go:151-159
                ok = False
            if ok:
                passing |= 1 << t
        if not have:
            f |= NODE["OPTIONS_EMPTY"]
        if have & ~passing:
            f |= NODE["OPTIONS_EXTRA"]
        if passing & ~have and int(prob["tmpl_limit_present"][m]) == 0xFFFFFFFF:
            f |= NODE["OPTIONS_MISSING"]
        nf[s] = f
    return pf, nf
