"""(CPU) The refusals of the audit's gate (include/kshost.h ksh_audit_gate / ksh_audit_gate_claimed; include/ksolve.h ks_audit_gate_dev / ks_audit_gate_batch_dev
where no device problem is needed):
  a) every refusal of the six passes that is not about a flag table -- the gate takes none --, reached through the gate with that pass alone in the mask: the code
     and the text the pass's own entry point gives for the same call, which tests/test_audit_refusals.py pins;
  b) where two passes of a mask refuse, or only a later one does, the earliest refusing pass's refusal;
  c) the gate's own three: an empty mask, an unknown bit, a NULL findings table with a capacity; and a requested pass without its array;
  d) nothing launched, nothing written: the out structs of every pass of the mask, poisoned before each refused call, are poisoned after it.
The problem and the handles are tests/test_audit_refusals.py's.  Runs the emulator in a subprocess (tests/simlib.py)."""
import pytest

import audit_harness as H
from test_audit_refusals import ARRAYS, PASSES

CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
import audit_limits_cases as LC
ks, kh = S.libs()
kh.ksh_last_error.restype = ctypes.c_char_p; ks.ks_last_error.restype = ctypes.c_char_p
PASSES, ARRAYS = json.loads(sys.argv[1])
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

kh.ksh_audit_gate.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
kh.ksh_audit_gate_claimed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
POISON = 0xA5

def gate_out(names, cap=0, table=False, without=()):
    # a gate out struct over poisoned pass structs; returns (struct, the bytes that must stay as they are)
    g = S._AuditGateOut(); arrays = []
    for w in names:
        if w in without: continue
        a = (S._AUDIT_PASSES[w]["Out"] * 1)(); ctypes.memset(a, POISON, ctypes.sizeof(a)); arrays.append(a); setattr(g, w, a)
    t = np.full(4 * max(1, cap), 0xA5A5A5A5, dtype=np.uint32); keep.append(t)
    g.findings, g.cap_findings = (t.ctypes.data if table else None), cap
    g.n_findings, g.truncated = 0xA5A5A5A5, 0xA5A5A5A5
    return g, arrays, t

def untouched(g, arrays, t):
    return all(bytes(a) == bytes([POISON]) * ctypes.sizeof(a) for a in arrays) and (t == 0xA5A5A5A5).all() and g.n_findings == 0xA5A5A5A5 and g.truncated == 0xA5A5A5A5

def mask_of(names):
    return sum(S.KS_AUDIT_PASS[w] for w in names)

def G_resident(key, names, handles, n, mask=None, **kw):
    g, arrays, t = gate_out(names, **kw)
    hv = (ctypes.c_void_p * max(1, len(handles)))(*handles) if handles is not None else None
    rc = kh.ksh_audit_gate(hv, n, mask_of(names) if mask is None else mask, ctypes.byref(g), None)
    out[key] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t))}

def G_claimed(key, names, h, ra, sq, **kw):
    g, arrays, t = gate_out(names, **kw)
    rc = kh.ksh_audit_gate_claimed(h, ctypes.byref(ra) if ra is not None else None, sq.ctypes.data if sq is not None else None, mask_of(names), ctypes.byref(g), None)
    out[key] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t))}

def own(key, what, resident, *args):
    # the pass's own entry point over the same call, with tables that fit
    Out = S._AUDIT_PASSES[what]["Out"]; first = what == "audit"
    name = "ksh_audit" if first else "ksh_audit_" + what
    outs = (Out * 2)(); o = outs[0]
    for x in outs:
        pf, nf = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32); keep.extend([pf, nf])
        x.cap_pods, x.pod_flags = 64, pf.ctypes.data
        if hasattr(x, "cap_nodes"): x.cap_nodes, x.node_flags = 64, nf.ctypes.data
    if resident:
        handles, n = args
        fn = getattr(kh, name); fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        hv = (ctypes.c_void_p * max(1, len(handles)))(*handles) if handles is not None else None
        rc = fn(hv, n, outs, None)
    else:
        h, ra, sq = args
        fn = getattr(kh, name + "_claimed"); fn.argtypes = [ctypes.c_void_p] * (4 if first else 5)
        rc = fn(h, ctypes.byref(ra) if ra is not None else None, *([] if first else [sq.ctypes.data if sq is not None else None]), ctypes.byref(o), None)
    out[key]["own"] = err(rc)

for what in PASSES:
    first = what == "audit"
    def R(case, handles, n):
        key = "%%s/resident/%%s" %% (what, case); G_resident(key, [what], handles, n); own(key, what, True, handles, n)
    def C(case, h, ra, sq):
        key = "%%s/claimed/%%s" %% (what, case); G_claimed(key, [what], h, ra, sq); own(key, what, False, h, ra, sq)
    R("null handles", None, 1)
    R("a null handle in the list", [None], 1)
    R("audit before solve", [fresh._h], 1)
    R("a derived what-if before its solve", [derived[0]._h], 1)
    R("the second of two before its solve", [solved._h, fresh._h], 2)
    C("null handle", None, claimed(), seq)
    C("null claimed", solved._h, None, seq)
    if not first:
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
    for a in ARRAYS:
        C("null array " + a, solved._h, claimed(**{a: None}), seq)

# ---- where two passes of a mask differ: the earliest refusing pass's refusal
G_claimed("order/spread accepts, firstfit refuses: null node_types", ["spread", "firstfit"], solved._h, claimed(node_types=None), seq)
G_claimed("order/firstfit alone: null unscheduled and null node_types", ["firstfit"], solved._h, claimed(unscheduled=None, node_types=None), seq)
G_claimed("order/first before firstfit: null unscheduled and null node_types", ["audit", "firstfit"], solved._h, claimed(unscheduled=None, node_types=None), seq)
G_claimed("order/all six: null node_it_state", PASSES, solved._h, claimed(node_it_state=None), seq)
G_resident("order/all six: the second of two before its solve", PASSES, [solved._h, fresh._h], 2)
# ---- the gate's own
G_resident("own/an empty mask", [], [solved._h], 1)
G_resident("own/an unknown bit", ["audit"], [solved._h], 1, mask=1 | 64)
G_resident("own/an unknown bit alone", [], [solved._h], 1, mask=1 << 31)
G_resident("own/null findings table, capacity 4", ["audit"], [solved._h], 1, cap=4, table=False)
G_resident("own/a requested pass without its array", ["audit", "limits"], [solved._h], 1, without=("limits",))
G_resident("own/two at once: an empty mask and audit before solve", [], [fresh._h], 1)
G_claimed("own/claimed: an empty mask", [], solved._h, claimed(), seq)
G_claimed("own/claimed: null findings table, capacity 4", ["audit"], solved._h, claimed(), seq, cap=4, table=False)
kh.ksh_audit_gate.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
out["own/null out"] = {"gate": err(kh.ksh_audit_gate((ctypes.c_void_p * 1)(solved._h), 1, 1, None, None)), "untouched": True}
# ---- accepted: the structs are written
g, arrays, t = gate_out(PASSES, cap=4, table=True)
rc = kh.ksh_audit_gate((ctypes.c_void_p * 1)(solved._h), 1, mask_of(PASSES), ctypes.byref(g), None)
out["accepted/resident"] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t)), "n_findings": int(g.n_findings), "n_pods": [int(a[0].n_pods) for a in arrays]}
g, arrays, t = gate_out(["audit"])
rc = kh.ksh_audit_gate_claimed(solved._h, ctypes.byref(claimed()), None, 1, ctypes.byref(g), None)      # the first pass alone takes no commit numbers
out["accepted/claimed, the first pass alone without pod_seq"] = {"gate": err(rc), "untouched": bool(untouched(g, arrays, t)), "n_findings": int(g.n_findings), "n_pods": [int(a[0].n_pods) for a in arrays]}
rc = kh.ksh_audit_gate(None, 0, 1, ctypes.byref(gate_out(["audit"])[0]), None)
out["accepted/n == 0"] = {"gate": err(rc)}
# ---- libksolve's own entry points, where no device problem is needed
ks.ks_audit_gate_dev.argtypes = [ctypes.c_void_p] * 3; ks.ks_audit_gate_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
room = (ctypes.c_uint64 * 256)(); one = (ctypes.c_void_p * 1)(ctypes.addressof(room)); none = (ctypes.c_void_p * 1)(None)
gate = (ctypes.c_uint32 * 64)(); gate[0] = 1      # ks_audit_gate{passes = FIRST, everything else null}
out["ks/dev: null problem"] = err(ks.ks_audit_gate_dev(None, None, gate), ks)
out["ks/dev: null gate"] = err(ks.ks_audit_gate_dev(room, None, None), ks)
out["ks/batch: null gate"] = err(ks.ks_audit_gate_batch_dev(one, 1, None), ks)
out["ks/batch: null problems, the pass's array null too"] = err(ks.ks_audit_gate_batch_dev(None, 1, gate), ks)
empty = (ctypes.c_uint32 * 64)()
out["ks/batch: an empty mask"] = err(ks.ks_audit_gate_batch_dev(one, 1, empty), ks)
unknown = (ctypes.c_uint32 * 64)(); unknown[0] = 64
out["ks/batch: an unknown bit"] = err(ks.ks_audit_gate_batch_dev(one, 1, unknown), ks)
capped = (ctypes.c_uint32 * 64)(); capped[0], capped[1] = 1, 4
out["ks/batch: null findings table, capacity 4"] = err(ks.ks_audit_gate_batch_dev(one, 1, capped), ks)
out["ks/batch: n == 0"] = err(ks.ks_audit_gate_batch_dev(None, 0, gate), ks)
ks.ks_audit_reduce_rows.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
out["ks/reduce_rows: null out"] = err(ks.ks_audit_reduce_rows(0, room, 4, None, None), ks)
out["ks/reduce_rows: null rows"] = err(ks.ks_audit_reduce_rows(0, None, 4, None, room), ks)
five = (ctypes.c_uint32 * 9)(5)
out["ks/reduce_rows: five fields"] = err(ks.ks_audit_reduce_rows(0, room, 4, five, room), ks)
for f in [solved, fresh] + derived:
    f.close()
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def recorded():
    return H.run_emulated(CHILD, [PASSES, ARRAYS])


INVALID, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("what", PASSES)
def test_a_passs_refusal_reaches_the_caller_through_the_gate_as_the_pass_gives_it(recorded, what):
    """With one pass in the mask the gate refuses what the pass refuses, with its code and text, and accepts what it accepts; a refused call writes nothing."""
    got = {k: v for k, v in recorded.items() if k.startswith(what + "/")}
    assert len(got) >= 30 and sum(1 for v in got.values() if v["own"][0] != 0) >= 15 and any(v["own"][0] == 0 for v in got.values()), len(got)
    wrong = {k: v for k, v in got.items() if v["gate"] != v["own"] or v["untouched"] != (v["own"][0] != 0)}
    assert not wrong, wrong


def test_the_earliest_refusing_pass_of_the_mask_wins(recorded):
    r = lambda k: tuple(recorded["order/" + k]["gate"])
    assert r("spread accepts, firstfit refuses: null node_types") == (INVALID, "claimed result: null array node_types")
    assert r("firstfit alone: null unscheduled and null node_types") == (INVALID, "claimed result: null array node_types")
    assert r("first before firstfit: null unscheduled and null node_types") == (INVALID, "claimed result: null array")      # (the first pass's, about the list only it reads)
    assert r("all six: null node_it_state") == (INVALID, "claimed result: null array node_it_state")
    assert r("all six: the second of two before its solve") == (INVALID, "audit before solve")
    assert all(v["untouched"] for k, v in recorded.items() if k.startswith("order/"))


def test_the_gates_own_refusals(recorded):
    r = lambda k: tuple(recorded["own/" + k]["gate"])
    assert r("an empty mask") == r("claimed: an empty mask") == r("two at once: an empty mask and audit before solve") == (INVALID, "audit gate: no pass requested")
    assert r("an unknown bit") == r("an unknown bit alone") == (INVALID, "audit gate: unknown pass")
    assert r("null findings table, capacity 4") == r("claimed: null findings table, capacity 4") == (INVALID, "audit gate: null findings table")
    assert r("a requested pass without its array") == r("null out") == (INVALID, "null argument")
    assert all(v["untouched"] for k, v in recorded.items() if k.startswith("own/"))


def test_an_accepted_call_writes_the_structs(recorded):
    a = recorded["accepted/resident"]
    assert a["gate"] == [0, ""] and not a["untouched"] and a["n_findings"] == 0 and a["n_pods"] == [5] * 6, a
    a = recorded["accepted/claimed, the first pass alone without pod_seq"]
    assert a["gate"] == [0, ""] and not a["untouched"] and a["n_findings"] == 0 and a["n_pods"] == [5], a
    assert recorded["accepted/n == 0"]["gate"] == [0, ""]


def test_libksolves_entry_points_refuse_without_a_device_problem(recorded):
    r = lambda k: tuple(recorded["ks/" + k])
    assert r("dev: null problem") == r("dev: null gate") == r("batch: null gate") == r("batch: null problems, the pass's array null too") == (INVALID, "null argument")
    assert r("batch: an empty mask") == (INVALID, "audit gate: no pass requested")
    assert r("batch: an unknown bit") == (INVALID, "audit gate: unknown pass")
    assert r("batch: null findings table, capacity 4") == (INVALID, "audit gate: null findings table")
    assert r("batch: n == 0") == (0, "")
    assert r("reduce_rows: null out") == r("reduce_rows: null rows") == (INVALID, "null argument")
    assert r("reduce_rows: five fields") == (INVALID, "audit reduce: more than four fields")
