"""(CPU) Every refusal of the six audit passes, resident and claimed, through the C ABI (include/kshost.h ksh_audit* / ksh_audit*_claimed; include/ksolve.h
ks_audit*_dev / ks_audit*_batch_dev for the refusals that need no device problem): the (code, message) of each, and which refusal wins where two apply at once.
EXPECTED was recorded from the commit before the five passes' host halves were folded into one path (csrc/ks_audit.inc's host half, host/api.cpp's audit entry
template) and holds unchanged after it: a caller sees the same refusals in the same order.  The sixth pass, added on that one path, has its entries from the commit
before the Python binding's six copies were folded into one table (karpenter_core_amd/scheduler.py _AUDIT_PASSES).  No kernel result is asserted here -- the calls that are accepted only
say so.  The problem is the smallest with a new node and an unscheduled pod: tests/audit_limits_cases.py's `capped` provisioner alone with five pods (two machines,
pods 3 and 4 unscheduled for the limit).
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import pytest

import audit_harness as H

PASSES = ["audit", "topology", "spread", "firstfit", "limits", "hostfit"]
ARRAYS = ["pod_node", "pod_stage", "pod_reason", "unscheduled", "node_pods_off", "node_pods", "node_tmpl", "node_types", "node_requests", "node_requests_present",
          "node_present", "node_complement", "node_mask", "node_gt", "node_lt", "node_it_state"]

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
OUT = {"audit": S._AuditOut, "topology": S._AuditTopologyOut, "spread": S._AuditSpreadOut, "firstfit": S._AuditFirstFitOut, "limits": S._AuditLimitsOut, "hostfit": S._AuditHostFitOut}
out = {}
def rec(key, rc, lib=kh):
    out[key] = [int(rc), "" if rc == S.KS_OK else (lib.ksh_last_error() if lib is kh else lib.ks_last_error()).decode()]

solved = S.FlatProblem(LC.capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR)
solved.solve(decode=False)
res = solved.result_arrays()
assert res["n_new"] == 2 and len(res["unscheduled"]) == 2, (res["n_new"], res["unscheduled"])
seq = np.ascontiguousarray(np.asarray(solved.pod_seq(), dtype=np.int32))
fresh = S.FlatProblem(LC.capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR)      # flattened, never solved
fresh.upload(0)
cold = S.FlatProblem(LC.capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR)       # flattened, never uploaded
snap, pn = LC.limited_snapshot()
derived = S.open_whatifs(S.ParsedProblem(snap), pn, LC.WHATIF_SETS[:1], derive=True)
d = solved.dims
keep = []

def table(Out, pods=True, nodes=True, cap=None):
    o = Out()
    pf, nf = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32); keep.extend([pf, nf])
    o.cap_pods = 64 if cap is None else cap
    o.pod_flags = pf.ctypes.data if pods else None
    if hasattr(o, "cap_nodes"):
        o.cap_nodes = 64 if cap is None else cap
        o.node_flags = nf.ctypes.data if nodes else None
    return o

def claimed(**edit):
    ra = S._ResultArrays()
    ra.n_pods, ra.n_existing, ra.n_new, ra.n_unscheduled = d["P"], d["E"], int(res["n_new"]), len(res["unscheduled"])
    ra.types_words, ra.n_resources, ra.n_keys = (d["T"] + 63) // 64, d["R"], d["K"]
    for name in ARRAYS:      # every array a table of its own, the ones no pass reads included
        a = np.zeros(4096, dtype=np.uint64)
        if name in res:
            src = np.ascontiguousarray(np.asarray(res[name]).reshape(-1)); a.view(np.uint8)[:src.nbytes] = src.view(np.uint8)
        keep.append(a); setattr(ra, name, a.ctypes.data)
    for k, v in edit.items():
        setattr(ra, k, v)
    return ra

for what in PASSES:
    Out = OUT[what]; has_nodes = hasattr(Out(), "cap_nodes"); first = what == "audit"
    name = "ksh_audit" if first else "ksh_audit_" + what
    resident, claimed_fn = getattr(kh, name), getattr(kh, name + "_claimed")
    resident.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    claimed_fn.argtypes = [ctypes.c_void_p] * (4 if first else 5)
    ms = (ctypes.c_double * 2)()
    def R(key, handles, n, o, ms=ms):
        hv = (ctypes.c_void_p * max(1, len(handles)))(*handles) if handles is not None else None
        rec("%%s/resident/%%s" %% (what, key), resident(hv, n, ctypes.byref(o) if o is not None else None, ms))
    def C(key, h, ra, sq, o, ms=ms):
        args = [h, ctypes.byref(ra) if ra is not None else None] + ([] if first else [sq.ctypes.data if sq is not None else None]) + [ctypes.byref(o) if o is not None else None, ms]
        rec("%%s/claimed/%%s" %% (what, key), claimed_fn(*args))
    # ---- resident
    R("n == 0, everything null", None, 0, None, None)
    R("n == 0", [solved._h], 0, table(Out))
    R("null handles", None, 1, table(Out))
    R("null outs", [solved._h], 1, None)
    R("a null handle in the list", [None], 1, table(Out))
    R("null pod table, capacity 1", [solved._h], 1, table(Out, pods=False, cap=1))
    if has_nodes:
        R("null node table, capacity 1", [solved._h], 1, table(Out, nodes=False, cap=1))
    R("null tables, capacity 0", [solved._h], 1, table(Out, pods=False, nodes=False, cap=0))
    R("audit before solve", [fresh._h], 1, table(Out))
    R("a derived what-if before its solve", [derived[0]._h], 1, table(Out))
    R("two at once: null pod table and audit before solve", [fresh._h], 1, table(Out, pods=False, cap=1))
    R("two at once: null handles and null pod table", None, 1, table(Out, pods=False, cap=1))
    R("accepted", [solved._h], 1, table(Out))
    R("accepted, ms null", [solved._h], 1, table(Out), None)
    # ---- claimed
    C("null handle", None, claimed(), seq, table(Out))
    C("null claimed", solved._h, None, seq, table(Out))
    if not first:
        C("null pod_seq", solved._h, claimed(), None, table(Out))
    C("null out", solved._h, claimed(), seq, None)
    C("null pod table, capacity 1", solved._h, claimed(), seq, table(Out, pods=False, cap=1))
    if has_nodes:
        C("null node table, capacity 1", solved._h, claimed(), seq, table(Out, nodes=False, cap=1))
    C("null tables, capacity 0", solved._h, claimed(), seq, table(Out, pods=False, nodes=False, cap=0))
    C("against a derived what-if", derived[0]._h, claimed(), seq, table(Out))
    C("two at once: derived what-if and null pod table", derived[0]._h, claimed(), seq, table(Out, pods=False, cap=1))
    C("two at once: derived what-if and dimensions", derived[0]._h, claimed(n_pods=d["P"] + 1), seq, table(Out))
    for dim in ("n_pods", "n_existing", "types_words", "n_resources", "n_keys"):
        C("dimensions: " + dim, solved._h, claimed(**{dim: getattr(claimed(), dim) + 1}), seq, table(Out))
    C("n_new above max_new_nodes", solved._h, claimed(n_new=d["P"] + 1), seq, table(Out))
    C("n_unscheduled above P", solved._h, claimed(n_unscheduled=d["P"] + 1), seq, table(Out))
    C("two at once: dimensions and n_new", solved._h, claimed(n_keys=d["K"] + 1, n_new=d["P"] + 1), seq, table(Out))
    C("two at once: n_new and n_unscheduled", solved._h, claimed(n_new=d["P"] + 1, n_unscheduled=d["P"] + 1), seq, table(Out))
    C("two at once: n_unscheduled and null pod_node", solved._h, claimed(n_unscheduled=d["P"] + 1, pod_node=None), seq, table(Out))
    C("two at once: null pod_node and null node_tmpl", solved._h, claimed(pod_node=None, node_tmpl=None), seq, table(Out))
    C("two at once: null node_it_state and null node_tmpl", solved._h, claimed(node_it_state=None, node_tmpl=None), seq, table(Out))
    for a in ARRAYS:
        C("null array " + a, solved._h, claimed(**{a: None}), seq, table(Out))
    C("null node arrays, n_new == 0", solved._h, claimed(n_new=0, **{a: None for a in ARRAYS if a.startswith("node_")}), seq, table(Out))
    C("null unscheduled, n_unscheduled == 0", solved._h, claimed(n_unscheduled=0, unscheduled=None), seq, table(Out))
    C("a claimed result for a handle never uploaded", cold._h, claimed(), seq, table(Out))
    C("accepted", solved._h, claimed(), seq, table(Out))
    C("accepted, ms null", solved._h, claimed(), seq, table(Out), None)
    # ---- libksolve's own entry points, where no device problem is needed
    dev, batch = getattr(ks, "ks_audit_dev" if first else "ks_audit_%%s_dev" %% what), getattr(ks, "ks_audit_batch_dev" if first else "ks_audit_%%s_batch_dev" %% what)
    dev.argtypes = [ctypes.c_void_p] * 3; batch.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    room = (ctypes.c_uint64 * 256)(); one = (ctypes.c_void_p * 1)(ctypes.addressof(room)); none = (ctypes.c_void_p * 1)(None)
    rec(what + "/ks_dev/null problem", dev(None, None, room), ks)
    rec(what + "/ks_dev/null problem, claimed given", dev(None, room, room), ks)
    rec(what + "/ks_dev/null problem and null out", dev(None, None, None), ks)
    rec(what + "/ks_batch/n == 0, everything null", batch(None, 0, None), ks)
    rec(what + "/ks_batch/null problems", batch(None, 1, one), ks)
    rec(what + "/ks_batch/null outs", batch(one, 1, None), ks)
    rec(what + "/ks_batch/a null problem in the list", batch(none, 1, one), ks)
    rec(what + "/ks_batch/two at once: a null problem and a null table", batch(none, 1, none), ks)
for f in [solved, fresh, cold] + derived:
    f.close()
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def recorded():
    return H.run_emulated(CHILD, [PASSES, ARRAYS])


ACCEPTED = (0, "")
DERIVED = "a claimed result is audited against a flattened problem, not against a what-if derived on the device"
# case -> (code, message) for every pass, or per pass (None: the pass has no such argument).  Recorded from the parent commit; KS_ERR_INVALID is -1, KS_ERR_UNSUPPORTED -2.
EXPECTED = {
    'claimed/a claimed result for a handle never uploaded': ACCEPTED,
    'claimed/accepted': ACCEPTED,
    'claimed/accepted, ms null': ACCEPTED,
    'claimed/against a derived what-if': (-2, DERIVED),
    'claimed/dimensions: n_existing': (-1, "claimed result: its dimensions are not the handle's"),
    'claimed/dimensions: n_keys': (-1, "claimed result: its dimensions are not the handle's"),
    'claimed/dimensions: n_pods': (-1, "claimed result: its dimensions are not the handle's"),
    'claimed/dimensions: n_resources': (-1, "claimed result: its dimensions are not the handle's"),
    'claimed/dimensions: types_words': (-1, "claimed result: its dimensions are not the handle's"),
    'claimed/n_new above max_new_nodes': (-1, 'claimed result: more new nodes than max_new_nodes'),
    'claimed/n_unscheduled above P': (-1, 'claimed result: more unscheduled pods than pods'),
    'claimed/null array node_complement': (-1, 'claimed result: null array node_complement'),
    'claimed/null array node_gt': (-1, 'claimed result: null array node_gt'),
    'claimed/null array node_it_state': {'audit': (-1, 'claimed result: null array node_it_state'), 'topology': ACCEPTED, 'spread': ACCEPTED, 'firstfit': (-1, 'claimed result: null array node_it_state'), 'limits': (-1, 'claimed result: null array node_it_state'), 'hostfit': (-1, 'claimed result: null array node_it_state')},
    'claimed/null array node_lt': (-1, 'claimed result: null array node_lt'),
    'claimed/null array node_mask': (-1, 'claimed result: null array node_mask'),
    'claimed/null array node_pods': ACCEPTED,
    'claimed/null array node_pods_off': ACCEPTED,
    'claimed/null array node_present': (-1, 'claimed result: null array node_present'),
    'claimed/null array node_requests': {'audit': (-1, 'claimed result: null array node_requests'), 'topology': ACCEPTED, 'spread': ACCEPTED, 'firstfit': (-1, 'claimed result: null array node_requests'), 'limits': (-1, 'claimed result: null array node_requests'), 'hostfit': (-1, 'claimed result: null array node_requests')},
    'claimed/null array node_requests_present': {'audit': (-1, 'claimed result: null array node_requests_present'), 'topology': ACCEPTED, 'spread': ACCEPTED, 'firstfit': (-1, 'claimed result: null array node_requests_present'), 'limits': (-1, 'claimed result: null array node_requests_present'), 'hostfit': (-1, 'claimed result: null array node_requests_present')},
    'claimed/null array node_tmpl': (-1, 'claimed result: null array node_tmpl'),
    'claimed/null array node_types': {'audit': (-1, 'claimed result: null array node_types'), 'topology': ACCEPTED, 'spread': ACCEPTED, 'firstfit': (-1, 'claimed result: null array node_types'), 'limits': (-1, 'claimed result: null array node_types'), 'hostfit': (-1, 'claimed result: null array node_types')},
    'claimed/null array pod_node': (-1, 'claimed result: null array'),
    'claimed/null array pod_reason': ACCEPTED,
    'claimed/null array pod_stage': (-1, 'claimed result: null array'),
    'claimed/null array unscheduled': {'audit': (-1, 'claimed result: null array'), 'topology': ACCEPTED, 'spread': ACCEPTED, 'firstfit': ACCEPTED, 'limits': ACCEPTED, 'hostfit': ACCEPTED},
    'claimed/null claimed': (-1, 'null argument'),
    'claimed/null handle': (-1, 'null argument'),
    'claimed/null node arrays, n_new == 0': ACCEPTED,
    'claimed/null node table, capacity 1': {'audit': (-1, 'null audit table'), 'topology': None, 'spread': None, 'firstfit': None, 'limits': (-1, 'null audit table'), 'hostfit': None},
    'claimed/null out': (-1, 'null audit table'),
    'claimed/null pod table, capacity 1': (-1, 'null audit table'),
    'claimed/null tables, capacity 0': ACCEPTED,
    'claimed/null unscheduled, n_unscheduled == 0': ACCEPTED,
    'claimed/two at once: derived what-if and dimensions': (-2, DERIVED),
    'claimed/two at once: derived what-if and null pod table': (-1, 'null audit table'),
    'claimed/two at once: dimensions and n_new': (-1, "claimed result: its dimensions are not the handle's"),
    'claimed/two at once: n_new and n_unscheduled': (-1, 'claimed result: more new nodes than max_new_nodes'),
    'claimed/two at once: n_unscheduled and null pod_node': (-1, 'claimed result: more unscheduled pods than pods'),
    'claimed/two at once: null node_it_state and null node_tmpl': (-1, 'claimed result: null array node_tmpl'),
    'claimed/two at once: null pod_node and null node_tmpl': (-1, 'claimed result: null array'),
    'ks_batch/a null problem in the list': (-1, 'null device problem'),
    'ks_batch/n == 0, everything null': ACCEPTED,
    'ks_batch/null outs': (-1, 'null argument'),
    'ks_batch/null problems': (-1, 'null argument'),
    'ks_batch/two at once: a null problem and a null table': (-1, 'null device problem'),
    'ks_dev/null problem': (-1, 'null argument'),
    'ks_dev/null problem and null out': (-1, 'null argument'),
    'ks_dev/null problem, claimed given': (-1, 'null argument'),
    'resident/a derived what-if before its solve': (-1, 'audit before solve'),
    'resident/a null handle in the list': (-1, 'audit before solve'),
    'resident/accepted': ACCEPTED,
    'resident/accepted, ms null': ACCEPTED,
    'resident/audit before solve': (-1, 'audit before solve'),
    'resident/n == 0': ACCEPTED,
    'resident/n == 0, everything null': ACCEPTED,
    'resident/null handles': (-1, 'null argument'),
    'resident/null node table, capacity 1': {'audit': (-1, 'null audit table'), 'topology': None, 'spread': None, 'firstfit': None, 'limits': (-1, 'null audit table'), 'hostfit': None},
    'resident/null outs': (-1, 'null argument'),
    'resident/null pod table, capacity 1': (-1, 'null audit table'),
    'resident/null tables, capacity 0': ACCEPTED,
    'resident/two at once: null handles and null pod table': (-1, 'null argument'),
    'resident/two at once: null pod table and audit before solve': (-1, 'null audit table'),
    'claimed/null pod_seq': {'audit': None, 'topology': (-1, 'null argument'), 'spread': (-1, 'null argument'), 'firstfit': (-1, 'null argument'), 'limits': (-1, 'null argument'), 'hostfit': (-1, 'null argument')},
}


def _key(what, case):
    return what + "/" + case


@pytest.mark.parametrize("what", PASSES)
def test_every_refusal_is_the_recorded_one(recorded, what):
    got = {k: tuple(v) for k, v in recorded.items() if k.startswith(what + "/")}
    want = {_key(what, case): (per[what] if isinstance(per, dict) else per) for case, per in EXPECTED.items()}
    want = {k: v for k, v in want.items() if v is not None}
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong


def test_a_pass_refuses_only_the_arrays_it_reads(recorded):
    """The first pass reads all fourteen of KS_AUDIT_SEGS (pod_seq is made by the entry point), topology and spread nine, first-fit, limits and host-fit all but the
    unscheduled list; pod_reason and the node -> pods CSR are read by none.  A null array outside a pass's set is accepted."""
    OK = 0
    node9, node13 = ["node_tmpl", "node_present", "node_complement", "node_mask", "node_gt", "node_lt"], [a for a in ARRAYS if a.startswith("node_") and not a.startswith("node_pods")]
    reads = {"audit": ["pod_node", "pod_stage", "unscheduled"] + node13, "topology": ["pod_node", "pod_stage"] + node9, "spread": ["pod_node", "pod_stage"] + node9,
             "firstfit": ["pod_node", "pod_stage"] + node13, "limits": ["pod_node", "pod_stage"] + node13, "hostfit": ["pod_node", "pod_stage"] + node13}
    for what in PASSES:
        for a in ARRAYS:
            code = recorded["%s/claimed/null array %s" % (what, a)][0]
            assert (code != OK) == (a in reads[what]), (what, a, code)
