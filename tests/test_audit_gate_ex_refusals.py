"""(CPU) The refusals of the audit's wide gate (include/kshost.h ksh_audit_gate_ex / ksh_audit_gate_ex_claimed; include/ksolve.h ks_audit_gate_ex_dev /
ks_audit_gate_ex_batch_dev where no device problem is needed), in the manner of tests/test_audit_gate_refusals.py:
  a) every refusal of the two new passes that is not about a flag table, reached through the wide gate with that pass alone in the mask: the code and the text the
     pass's own entry point gives for the same call;
  b) the mask order: the earliest refusing pass's refusal wins, and the null pod_reason refusal -- the eighth pass's -- comes last;
  c) the growth rule: a struct_size that ends before `stages` makes bit 64 unknown, one that ends before `reasons` bit 128; bit 256 is unknown whatever the size; a
     struct_size below the struct's first version; a requested pass without its array;
  d) nothing launched, nothing written: the out structs of every pass of the mask, poisoned before each refused call, are poisoned after it;
  e) bit 64 through the four OLD entry points is still "audit gate: unknown pass".
The problem and the handles are tests/test_audit_refusals.py's.  Runs the emulator in a subprocess (tests/simlib.py)."""
import pytest

import audit_harness as H
from test_audit_refusals import ARRAYS

NEW = ["stages", "reasons"]

CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
import audit_limits_cases as LC
ks, kh = S.libs()
kh.ksh_last_error.restype = ctypes.c_char_p; ks.ks_last_error.restype = ctypes.c_char_p
NEW, ARRAYS = json.loads(sys.argv[1])
ALL = list(S.AUDIT_GATE_ALL)
out = {}
err = lambda rc, lib=kh: [int(rc), "" if rc == S.KS_OK else (lib.ksh_last_error() if lib is kh else lib.ks_last_error()).decode()]

solved = S.FlatProblem(LC.capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR)
solved.solve(decode=False)
res = solved.result_arrays()
seq = np.ascontiguousarray(np.asarray(solved.pod_seq(), dtype=np.int32))
fresh = S.FlatProblem(LC.capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR); fresh.upload(0)      # flattened, never solved
snap, pn = LC.limited_snapshot()
derived = S.open_whatifs(S.ParsedProblem(snap), pn, LC.WHATIF_SETS[:1], derive=True)
d = solved.dims
keep = []

def claimed(**edit):
    ra = S._ResultArrays()
    ra.n_pods, ra.n_existing, ra.n_new, ra.n_unscheduled = d["P"], d["E"], int(res["n_new"]), len(res["unscheduled"])
    ra.types_words, ra.n_resources, ra.n_keys = (d["T"] + 63) // 64, d["R"], d["K"]
    for name in ARRAYS:
        a = np.zeros(4096, dtype=np.uint64)
        if name in res:
            src = np.ascontiguousarray(np.asarray(res[name]).reshape(-1)); a.view(np.uint8)[:src.nbytes] = src.view(np.uint8)
        keep.append(a); setattr(ra, name, a.ctypes.data)
    for k, v in edit.items():
        setattr(ra, k, v)
    return ra

for fn in (kh.ksh_audit_gate_ex, kh.ksh_audit_gate):
    fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
for fn in (kh.ksh_audit_gate_ex_claimed, kh.ksh_audit_gate_claimed):
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
POISON = 0xA5
Gate = S._AuditGateExOut

def gate_out(names, cap=0, table=False, without=(), size=None):
    # a wide gate out struct over poisoned pass structs; returns (struct, the arrays that must stay as they are, the findings table)
    g = Gate(); arrays = []
    g.struct_size = ctypes.sizeof(Gate) if size is None else size
    for w in names:
        if w in without: continue
        a = (S._AUDIT_PASSES_EX[w]["Out"] * 1)(); ctypes.memset(a, POISON, ctypes.sizeof(a)); arrays.append(a); setattr(g, w, a)
    t = np.full(4 * max(1, cap), 0xA5A5A5A5, dtype=np.uint32); keep.append(t)
    g.findings, g.cap_findings = (t.ctypes.data if table else None), cap
    g.n_findings, g.truncated = 0xA5A5A5A5, 0xA5A5A5A5
    return g, arrays, t

def untouched(g, arrays, t):
    return all(bytes(a) == bytes([POISON]) * ctypes.sizeof(a) for a in arrays) and (t == 0xA5A5A5A5).all() and g.n_findings == 0xA5A5A5A5 and g.truncated == 0xA5A5A5A5

def mask_of(names):
    return sum(S.KS_AUDIT_PASS_EX[w] for w in names)

def G_resident(key, names, handles, n, mask=None, **kw):
    g, arrays, t = gate_out(names, **kw)
    hv = (ctypes.c_void_p * max(1, len(handles)))(*handles) if handles is not None else None
    rc = kh.ksh_audit_gate_ex(hv, n, mask_of(names) if mask is None else mask, ctypes.byref(g), None)
    out[key] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t))}

def G_claimed(key, names, h, ra, sq, **kw):
    g, arrays, t = gate_out(names, **kw)
    rc = kh.ksh_audit_gate_ex_claimed(h, ctypes.byref(ra) if ra is not None else None, sq.ctypes.data if sq is not None else None, mask_of(names), ctypes.byref(g), None)
    out[key] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t))}

def own(key, what, resident, *args):
    # the pass's own entry point over the same call, with tables that fit
    Out = S._AUDIT_PASSES_EX[what]["Out"]; takes_seq = S._AUDIT_PASSES_EX[what]["seq"]
    name = "ksh_audit_" + what
    outs = (Out * 2)(); o = outs[0]
    for x in outs:
        pf = np.zeros(64, dtype=np.uint32); keep.append(pf)
        x.cap_pods, x.pod_flags = 64, pf.ctypes.data
    if resident:
        handles, n = args
        fn = getattr(kh, name); fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        hv = (ctypes.c_void_p * max(1, len(handles)))(*handles) if handles is not None else None
        rc = fn(hv, n, outs, None)
    else:
        h, ra, sq = args
        fn = getattr(kh, name + "_claimed"); fn.argtypes = [ctypes.c_void_p] * (5 if takes_seq else 4)
        rc = fn(h, ctypes.byref(ra) if ra is not None else None, *([sq.ctypes.data if sq is not None else None] if takes_seq else []), ctypes.byref(o), None)
    out[key]["own"] = err(rc)

for what in NEW:
    takes_seq = S._AUDIT_PASSES_EX[what]["seq"]
    def R(case, handles, n):
        key = "%%s/resident/%%s" %% (what, case); G_resident(key, [what], handles, n); own(key, what, True, handles, n)
    def C(case, h, ra, sq):
        key = "%%s/claimed/%%s" %% (what, case); G_claimed(key, [what], h, ra, sq); own(key, what, False, h, ra, sq)
    R("null handles", None, 1)
    R("a null handle in the list", [None], 1)
    R("audit before solve", [fresh._h], 1)
    R("a derived what-if before its solve", [derived[0]._h], 1)
    R("the second of two before its solve", [solved._h, fresh._h], 2)
    R("accepted", [solved._h], 1)
    C("accepted", solved._h, claimed(), seq)
    C("null handle", None, claimed(), seq)
    C("null claimed", solved._h, None, seq)
    if takes_seq:
        C("null pod_seq", solved._h, claimed(), None)
    C("against a derived what-if", derived[0]._h, claimed(), seq)
    C("two at once: derived what-if and dimensions", derived[0]._h, claimed(n_pods=d["P"] + 1), seq)
    for dim in ("n_pods", "n_existing", "types_words", "n_resources", "n_keys"):
        C("dimensions: " + dim, solved._h, claimed(**{dim: getattr(claimed(), dim) + 1}), seq)
    C("n_new above max_new_nodes", solved._h, claimed(n_new=d["P"] + 1), seq)
    C("n_unscheduled above P", solved._h, claimed(n_unscheduled=d["P"] + 1), seq)
    C("two at once: n_new and n_unscheduled", solved._h, claimed(n_new=d["P"] + 1, n_unscheduled=d["P"] + 1), seq)
    C("two at once: n_unscheduled and null pod_node", solved._h, claimed(n_unscheduled=d["P"] + 1, pod_node=None), seq)
    C("two at once: null node_it_state and null node_tmpl", solved._h, claimed(node_it_state=None, node_tmpl=None), seq)
    C("two at once: null pod_reason and null pod_stage", solved._h, claimed(pod_reason=None, pod_stage=None), seq)
    for a in ARRAYS:
        C("null array " + a, solved._h, claimed(**{a: None}), seq)

# ---- the mask order: the earliest refusing pass's refusal; the null pod_reason refusal comes last
G_claimed("order/stages refuses, reasons would too: null node_types and null pod_reason", ["stages", "reasons"], solved._h, claimed(node_types=None, pod_reason=None), seq)
G_claimed("order/hostfit before stages before reasons: null node_it_state and null pod_reason", ["hostfit", "stages", "reasons"], solved._h, claimed(node_it_state=None, pod_reason=None), seq)
G_claimed("order/all eight: null pod_reason alone", ALL, solved._h, claimed(pod_reason=None), seq)
G_claimed("order/all eight: null unscheduled and null pod_reason", ALL, solved._h, claimed(unscheduled=None, pod_reason=None), seq)
G_claimed("order/first and reasons: null pod_reason, no pod_seq", ["audit", "reasons"], solved._h, claimed(pod_reason=None), None)
G_claimed("order/first and stages: no pod_seq", ["audit", "stages"], solved._h, claimed(), None)
G_resident("order/all eight: the second of two before its solve", ALL, [solved._h, fresh._h], 2)
# a null pod_reason is nobody's business unless the eighth pass is requested
g, arrays, t = gate_out(["audit", "stages"])
rc = kh.ksh_audit_gate_ex_claimed(solved._h, ctypes.byref(claimed(pod_reason=None)), seq.ctypes.data, mask_of(["audit", "stages"]), ctypes.byref(g), None)
out["accepted/first and stages with a null pod_reason"] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t)), "n_pods": [int(a[0].n_pods) for a in arrays]}
g, arrays, t = gate_out(["audit", "reasons"])
rc = kh.ksh_audit_gate_ex_claimed(solved._h, ctypes.byref(claimed()), None, mask_of(["audit", "reasons"]), ctypes.byref(g), None)      # the two passes that take no commit numbers
out["accepted/first and reasons without pod_seq"] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t)), "n_pods": [int(a[0].n_pods) for a in arrays]}
g, arrays, t = gate_out(ALL, cap=4, table=True)
rc = kh.ksh_audit_gate_ex((ctypes.c_void_p * 1)(solved._h), 1, mask_of(ALL), ctypes.byref(g), None)
out["accepted/resident, all eight"] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t)), "n_findings": int(g.n_findings), "n_pods": [int(a[0].n_pods) for a in arrays]}
rc = kh.ksh_audit_gate_ex(None, 0, 64, ctypes.byref(gate_out(["stages"])[0]), None)
out["accepted/n == 0"] = {"gate": err(rc)}
# ---- the growth rule
before_stages, before_reasons = Gate.stages.offset, Gate.reasons.offset
G_resident("size/ends before stages: bit 64", ["stages"], [solved._h], 1, size=before_stages)
G_resident("size/ends inside stages: bit 64", ["stages"], [solved._h], 1, size=before_stages + 4)
G_resident("size/ends before reasons: bit 128", ["reasons"], [solved._h], 1, size=before_reasons)
G_resident("size/ends before reasons: bit 64 is known", ["stages"], [solved._h], 1, size=before_reasons)
G_resident("size/ends before stages: the six are known", ["audit", "hostfit"], [solved._h], 1, size=before_stages)
G_resident("size/below the first version", ["audit"], [solved._h], 1, size=before_stages - 8)
G_resident("size/zero", ["audit"], [solved._h], 1, size=0)
G_resident("size/larger than today's: bit 256", ["audit"], [solved._h], 1, mask=1 | 256, size=ctypes.sizeof(Gate) + 8)
G_resident("own/bit 256", ["audit"], [solved._h], 1, mask=1 | 256)
G_resident("own/bit 256 alone", [], [solved._h], 1, mask=256)
G_resident("own/an empty mask", [], [solved._h], 1)
G_resident("own/null findings table, capacity 4", ["stages"], [solved._h], 1, cap=4, table=False)
G_resident("own/stages requested without its array", ["audit", "stages"], [solved._h], 1, without=("stages",))
G_resident("own/reasons requested without its array", ["reasons"], [solved._h], 1, without=("reasons",))
G_claimed("own/claimed: bit 64 with a struct that ends before stages", ["stages"], solved._h, claimed(), seq, size=before_stages)
out["own/null out"] = {"gate": err(kh.ksh_audit_gate_ex((ctypes.c_void_p * 1)(solved._h), 1, 64, None, None)), "untouched": True}
# ---- bit 64 through the four old entry points
old = S._AuditGateOut(); a6 = (S._AuditOut * 1)(); ctypes.memset(a6, POISON, ctypes.sizeof(a6)); old.audit = a6; old.n_findings = 0xA5A5A5A5
out["old/ksh_audit_gate: bit 64"] = err(kh.ksh_audit_gate((ctypes.c_void_p * 1)(solved._h), 1, 1 | 64, ctypes.byref(old), None))
out["old/ksh_audit_gate_claimed: bit 64"] = err(kh.ksh_audit_gate_claimed(solved._h, ctypes.byref(claimed()), seq.ctypes.data, 1 | 64, ctypes.byref(old), None))
out["old/untouched"] = bool(bytes(a6) == bytes([POISON]) * ctypes.sizeof(a6) and old.n_findings == 0xA5A5A5A5)
ks.ks_audit_gate_dev.argtypes = [ctypes.c_void_p] * 3; ks.ks_audit_gate_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
ks.ks_audit_gate_ex_dev.argtypes = [ctypes.c_void_p] * 3; ks.ks_audit_gate_ex_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
room = (ctypes.c_uint64 * 256)(); one = (ctypes.c_void_p * 1)(ctypes.addressof(room))
unknown = (ctypes.c_uint32 * 64)(); unknown[0] = 64      # ks_audit_gate{passes = 64}
out["old/ks_audit_gate_batch_dev: bit 64"] = err(ks.ks_audit_gate_batch_dev(one, 1, unknown), ks)
out["old/ks_audit_gate_dev: bit 64"] = err(ks.ks_audit_gate_dev(room, None, unknown), ks)
# ---- libksolve's wide entry points, where no device problem is needed: ks_audit_gate_ex{struct_size, passes, cap_findings, ...}
SIZE = 120      # sizeof(ks_audit_gate_ex): tests/test_audit_gate_ex_binding.py holds it against the header
def ex(size, passes, cap=0):
    g = (ctypes.c_uint32 * 64)(); g[0], g[1], g[2] = size, passes, cap
    return g
out["ks/dev: null problem"] = err(ks.ks_audit_gate_ex_dev(None, None, ex(SIZE, 64)), ks)
out["ks/dev: null gate"] = err(ks.ks_audit_gate_ex_dev(room, None, None), ks)
out["ks/batch: null gate"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, None), ks)
out["ks/batch: null problems, the pass's array null too"] = err(ks.ks_audit_gate_ex_batch_dev(None, 1, ex(SIZE, 64)), ks)
out["ks/batch: an empty mask"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(SIZE, 0)), ks)
out["ks/batch: bit 256"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(SIZE, 256)), ks)
out["ks/batch: bit 64, the struct ends before stages"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(SIZE - 16, 64)), ks)
out["ks/batch: bit 128, the struct ends before reasons"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(SIZE - 8, 128)), ks)
out["ks/batch: bit 64 known, its array null"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(SIZE - 8, 64)), ks)
out["ks/batch: struct_size 0"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(0, 1)), ks)
out["ks/batch: null findings table, capacity 4"] = err(ks.ks_audit_gate_ex_batch_dev(one, 1, ex(SIZE, 64, 4)), ks)
out["ks/batch: n == 0"] = err(ks.ks_audit_gate_ex_batch_dev(None, 0, ex(SIZE, 192)), ks)
for f in [solved, fresh] + derived:
    f.close()
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def recorded():
    return H.run_emulated(CHILD, [NEW, ARRAYS])


INVALID, UNSUPPORTED = -1, -2
UNKNOWN = (INVALID, "audit gate: unknown pass")
NO_REASON = (INVALID, "claimed result: null array pod_reason")


@pytest.mark.parametrize("what", NEW)
def test_a_new_passs_refusal_reaches_the_caller_through_the_wide_gate_as_the_pass_gives_it(recorded, what):
    """With one pass in the mask the gate refuses what the pass refuses, with its code and text, and accepts what it accepts; a refused call writes nothing."""
    got = {k: v for k, v in recorded.items() if k.startswith(what + "/")}
    assert len(got) >= 30 and sum(1 for v in got.values() if v["own"][0] != 0) >= 15 and sum(1 for v in got.values() if v["own"][0] == 0) >= 2, len(got)
    wrong = {k: v for k, v in got.items() if v["gate"] != v["own"] or v["untouched"] != (v["own"][0] != 0)}
    assert not wrong, wrong
    if what == "reasons":
        assert tuple(got["reasons/claimed/null array pod_reason"]["gate"]) == NO_REASON
        assert tuple(got["reasons/claimed/two at once: null pod_reason and null pod_stage"]["gate"]) == (INVALID, "claimed result: null array")


def test_the_earliest_refusing_pass_wins_and_the_null_pod_reason_refusal_comes_last(recorded):
    r = lambda k: tuple(recorded["order/" + k]["gate"])
    assert r("stages refuses, reasons would too: null node_types and null pod_reason") == (INVALID, "claimed result: null array node_types")
    assert r("hostfit before stages before reasons: null node_it_state and null pod_reason") == (INVALID, "claimed result: null array node_it_state")
    assert r("all eight: null pod_reason alone") == NO_REASON
    assert r("all eight: null unscheduled and null pod_reason") == (INVALID, "claimed result: null array")      # (the first pass's, about the list only it reads)
    assert r("first and reasons: null pod_reason, no pod_seq") == NO_REASON
    assert r("first and stages: no pod_seq") == (INVALID, "null argument")
    assert r("all eight: the second of two before its solve") == (INVALID, "audit before solve")
    assert all(v["untouched"] for k, v in recorded.items() if k.startswith("order/"))


def test_struct_size_decides_which_passes_a_caller_can_ask_for(recorded):
    r = lambda k: tuple(recorded["size/" + k]["gate"])
    assert r("ends before stages: bit 64") == r("ends inside stages: bit 64") == r("ends before reasons: bit 128") == r("larger than today's: bit 256") == UNKNOWN
    assert r("ends before reasons: bit 64 is known") == r("ends before stages: the six are known") == (0, "")
    assert r("below the first version") == r("zero") == (INVALID, "audit gate: struct_size is less than the struct's first version")
    assert all(v["untouched"] == (v["gate"][0] != 0) for k, v in recorded.items() if k.startswith("size/"))


def test_the_wide_gates_own_refusals(recorded):
    r = lambda k: tuple(recorded["own/" + k]["gate"])
    assert r("bit 256") == r("bit 256 alone") == r("claimed: bit 64 with a struct that ends before stages") == UNKNOWN
    assert r("an empty mask") == (INVALID, "audit gate: no pass requested")
    assert r("null findings table, capacity 4") == (INVALID, "audit gate: null findings table")
    assert r("stages requested without its array") == r("reasons requested without its array") == r("null out") == (INVALID, "null argument")
    assert all(v["untouched"] for k, v in recorded.items() if k.startswith("own/"))


def test_an_accepted_call_writes_the_structs(recorded):
    a = recorded["accepted/resident, all eight"]
    assert a["gate"] == [0, ""] and not a["untouched"] and a["n_findings"] == 0 and a["n_pods"] == [5] * 8, a
    for k in ("accepted/first and stages with a null pod_reason", "accepted/first and reasons without pod_seq"):
        a = recorded[k]
        assert a["gate"] == [0, ""] and not a["untouched"] and a["n_pods"] == [5, 5], (k, a)
    assert recorded["accepted/n == 0"]["gate"] == [0, ""]


def test_bit_64_through_the_four_old_entry_points_is_still_refused(recorded):
    for k in ("ksh_audit_gate", "ksh_audit_gate_claimed", "ks_audit_gate_batch_dev", "ks_audit_gate_dev"):
        assert tuple(recorded["old/%s: bit 64" % k]) == UNKNOWN, k
    assert recorded["old/untouched"] is True


def test_libksolves_wide_entry_points_refuse_without_a_device_problem(recorded):
    r = lambda k: tuple(recorded["ks/" + k])
    assert r("dev: null problem") == r("dev: null gate") == r("batch: null gate") == r("batch: null problems, the pass's array null too") == r("batch: bit 64 known, its array null") == (INVALID, "null argument")
    assert r("batch: an empty mask") == (INVALID, "audit gate: no pass requested")
    assert r("batch: bit 256") == r("batch: bit 64, the struct ends before stages") == r("batch: bit 128, the struct ends before reasons") == UNKNOWN
    assert r("batch: struct_size 0") == (INVALID, "audit gate: struct_size is less than the struct's first version")
    assert r("batch: null findings table, capacity 4") == (INVALID, "audit gate: null findings table")
    assert r("batch: n == 0") == (0, "")
