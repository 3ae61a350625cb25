"""(CPU) The audit's gate (include/ksolve.h ks_audit_gate_dev / ks_audit_gate_batch_dev, kshost.h ksh_audit_gate / ksh_audit_gate_claimed; kernels in
karpenter_core_amd/csrc/ks_audit_reduce.inc) on the emulator, against the six passes' own calls -- the reference here: they are unchanged by the gate and pinned
against the literal references by their own suites:
  a) behind EVERY call the passes' cases modules make (tests/audit_*_cases.py: the genuine results, each pass's tamper matrix, the claimed results with indices out of
     range, the shapes where a pass takes another path, the limited snapshot's what-ifs as a batch) the gate with all six passes and with three sub-masks -- a single
     pass, first + firstfit + hostfit, limits alone -- says what the six calls say: every totals field equal, `findings` the non-zero entries of the six flag tables
     in the stated order, `clean` exactly when all six tables are zero, and twice the same bytes (tests/audit_gate_checks.py);
  b) the batch form over mixed sizes, an empty problem among them; the claimed form;
  c) findings at the cap: a claimed result of 640 pods, each flagged by the first pass, so that the findings span three workgroups; caps 0, 1, n - 1, n, n + 1.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import pytest

import audit_harness as H

MODULES = ["audit_cases", "audit_topo_cases", "audit_spread_cases", "audit_firstfit_cases", "audit_limits_cases", "audit_hostfit_cases"]
RUNS = ["run_tamper_matrix", "run_range_cases", "run_shapes", "run_shape_tampers", "run_one_sided", "run_whatifs"]      # what a cases module has of these, it runs

CHILD = r"""
import importlib, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
import audit_gate_checks as G
import audit_spread_cases as SC, audit_topo_cases as TC
modules, runs = json.loads(sys.argv[1])
out = {"modules": {}}
for name in modules:
    M = importlib.import_module(name)
    rec = G.Recorder(S, masks=(None,) + G.SUB_MASKS)
    report = []
    try:
        for fn in runs:
            if hasattr(M, fn):
                got = getattr(M, fn)(S)      # [(case, True or what differs)]; run_whatifs asserts for itself and returns its summaries
                report += [[fn, True]] if fn == "run_whatifs" else [[fn + ": " + str(r[0]), r[1] if r[1] is True else str(r[1])[:600]] for r in got]
    except Exception as e:
        report.append(["raised", repr(e)[:600]])
    finally:
        rec.remove()
    out["modules"][name] = {"report": report, "compared": len(rec.seen), "with_findings": sum(1 for s in rec.seen if s[3]), "claimed": sum(1 for s in rec.seen if s[2]),
                            "batches": sum(1 for s in rec.seen if s[1] > 1)}

def section(name, fn):
    try:
        out[name] = fn()
    except Exception as e:
        out[name] = {"error": repr(e)[:900]}

def mixed_batch():
    # every cases module's tamper problem, an empty problem and 640 zonal pods, solved one by one: the batch form over the lot, then over its reverse
    probs = [importlib.import_module(m) for m in modules]
    probs = [M.tamper_problem() if hasattr(M, "tamper_problem") else M.capped_problem() for M in probs] + [TC.plain(pods=0), SC.zonal(pods=640)]
    flats = [S.FlatProblem(p) for p in probs]
    for f in flats:
        f.solve(decode=False)
    six, g = G.gate_against_calls(S, flats)
    G.gate_against_calls(S, flats[::-1], masks=(None,))
    sizes = [f.dims["P"] for f in flats]
    for f in flats:
        f.close()
    return {"sizes": sizes, "clean": g["clean"], "n": len(flats)}

def claimed_form():
    import audit_hostfit_cases as HC
    f = S.FlatProblem(HC.tamper_problem()); f.solve(decode=False)
    found = []
    for name, r, s, want in HC.tampers(f.result_arrays(), f.pod_seq()):
        six, g = G.gate_against_calls(S, [f], r, s)
        one = f.audit_gate(r, s)
        assert one["passes"]["hostfit"] == g["passes"]["hostfit"][0] and one["findings"].tobytes() == g["findings"].tobytes()
        hostfit = {int(x["index"]): int(x["flags"]) for x in g["findings"] if x["where"] == (5 << 8)}
        assert hostfit == want, (name, hostfit, want)
        found.append(g["n_findings"])
    f.close()
    return {"found": found}

def at_the_cap():
    f = S.FlatProblem(SC.zonal(pods=640)); f.solve(decode=False)
    r, s = G.all_flagged_claim(S, f)
    got = G.findings_at_the_cap(S, f, r, s)
    f.close()
    return {"caps": got}

section("mixed_batch", mixed_batch)
section("claimed_form", claimed_form)
section("at_the_cap", at_the_cap)
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [MODULES, RUNS])


@pytest.mark.parametrize("module", MODULES)
def test_the_gate_says_what_the_six_calls_say_behind_every_call_of_a_cases_module(emulated, module):
    """A difference between the gate and the six calls is an AssertionError inside the pass's call: the cases module reports it as a failed case, or it ends the module's
    run ("raised").  Every module audits genuine and tampered results, so some comparisons were over clean tables and some over findings, some resident, some claimed."""
    got = emulated["modules"][module]
    print(module, got["compared"], got["with_findings"], got["claimed"], got["batches"])
    bad = [r for r in got["report"] if r[1] is not True]
    assert not bad, bad[:3]
    assert got["report"] and got["compared"] >= 8 and 0 < got["with_findings"] < got["compared"] and 0 < got["claimed"] < got["compared"], got


def test_whatif_batches_derived_on_the_device_were_among_them(emulated):
    """tests/audit_limits_cases.py's run_whatifs audits the limited snapshot's what-ifs as batches, flattened one by one and derived on the device."""
    assert emulated["modules"]["audit_limits_cases"]["batches"] >= 2, emulated["modules"]["audit_limits_cases"]


def test_the_batch_form_over_mixed_sizes_with_an_empty_problem(emulated):
    got = emulated["mixed_batch"]
    assert "error" not in got, got
    assert got["n"] == len(MODULES) + 2 and 0 in got["sizes"] and 640 in got["sizes"] and got["clean"] is True, got


def test_the_claimed_form_lists_exactly_the_sixth_passs_findings(emulated):
    got = emulated["claimed_form"]
    assert "error" not in got, got
    assert len(got["found"]) == 4 and all(n >= 1 for n in got["found"]), got


def test_findings_at_the_cap(emulated):
    got = emulated["at_the_cap"]
    assert "error" not in got, got
    assert got["caps"] == [[0, 640, True], [1, 640, True], [639, 640, True], [640, 640, False], [641, 640, False]], got
