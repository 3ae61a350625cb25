"""(CPU) The audit's WIDE gate (include/ksolve.h ks_audit_gate_ex_dev / ks_audit_gate_ex_batch_dev, kshost.h ksh_audit_gate_ex / ksh_audit_gate_ex_claimed: all eight
passes in one call, the seventh without its host wait) on the emulator, against the eight passes' own calls -- the reference here: they are unchanged by the gate and
pinned against the literal references by their own suites (tests/audit_gate_ex_checks.py):
  a) behind EVERY call the two new passes' cases modules make (tests/audit_stages_cases.py, tests/audit_reasons_cases.py: run_tamper_matrix, run_shapes,
     derived_whatifs) the wide gate with all eight passes and with four sub-masks -- each new pass alone, first + stages + reasons (in the claimed form both side arrays
     in one upload), firstfit + stages (the fourth pass's kernels back to back in two roles) -- says what the eight calls say: every totals field equal, `findings` the
     non-zero entries of the eight pod and node tables in the stated order, `clean` exactly when all are zero, twice the same bytes; and over the six the wide gate
     and the old one answer alike;
  b) a mixed batch -- a problem whose pods relax, one in which nothing relaxes, an empty one, the smallest whose pods stay unscheduled -- forward and reversed: the
     non-relaxing problems' words are what each says alone, whatever its neighbours do;
  c) the four SILENT edits of the stages matrix and the nine reasons edits: the six-pass gate is clean on each, the wide gate lists exactly the passes' own flagged
     pods under pass 6 or 7 and is not clean;
  d) the shapes at which the tail can go wrong: P = 1, P = 257, no pod relaxed at all, M = 9 templates;
  e) a findings cap that ends inside pass 6's records.
Runs the emulator in a subprocess: its build replaces the two libraries for the whole process (tests/simlib.py)."""
import pytest

import audit_harness as H

MODULES = ["audit_stages_cases", "audit_reasons_cases"]
RUNS = ["run_tamper_matrix", "run_shapes", "derived_whatifs"]      # what a cases module has of these, it runs

CHILD = r"""
import importlib, json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import audit_gate_ex_checks as X
modules, runs = json.loads(sys.argv[1])
out = {"modules": {}}
for name in modules:
    M = importlib.import_module(name)
    rec = X.Recorder(S, masks=(None,) + X.EX_MASKS)
    report = []
    try:
        for fn in runs:
            if hasattr(M, fn):
                got = getattr(M, fn)(S)      # [(case, True or what differs)]; derived_whatifs asserts for itself and returns its summaries
                report += [[fn, True]] if fn == "derived_whatifs" else [[fn + ": " + str(r[0]), r[1] if r[1] is True else str(r[1])[:600]] for r in got]
    except Exception as e:
        report.append(["raised", repr(e)[:600]])
    finally:
        rec.remove()
    out["modules"][name] = {"report": report, "compared": len(rec.seen), "with_findings": sum(1 for s in rec.seen if s[3]), "new_pass_findings": sum(1 for s in rec.seen if s[4]),
                            "claimed": sum(1 for s in rec.seen if s[2]), "batches": sum(1 for s in rec.seen if s[1] > 1)}

def section(name, fn):
    try:
        out[name] = fn()
    except Exception as e:
        out[name] = {"error": repr(e)[:900]}

section("mixed_batch", lambda: X.mixed_batch_both_ways(S))
section("silent_edits", lambda: {"edits": X.silent_edits(S)})
section("tail_shapes", lambda: {"shapes": X.tail_shapes(S)})
section("cap", lambda: {"counts": X.cap_inside_pass_six(S)})
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def emulated():
    return H.run_emulated(CHILD, [MODULES, RUNS])


@pytest.mark.parametrize("module", MODULES)
def test_the_wide_gate_says_what_the_eight_calls_say_behind_every_call_of_a_cases_module(emulated, module):
    """A difference between the gate and the eight calls is an AssertionError inside the pass's call: the cases module reports it as a failed case, or it ends the
    module's run ("raised").  Both modules audit genuine and tampered results: some comparisons over clean tables, some over findings of the two new passes."""
    got = emulated["modules"][module]
    print(module, got)
    bad = [r for r in got["report"] if r[1] is not True]
    assert not bad, bad[:3]
    assert got["report"] and got["compared"] >= 20 and 0 < got["new_pass_findings"] <= got["with_findings"] < got["compared"] and 0 < got["claimed"] < got["compared"], got


def test_the_derived_whatifs_of_the_stages_cases_went_through_as_batches(emulated):
    assert emulated["modules"]["audit_stages_cases"]["batches"] >= 2 and ["derived_whatifs", True] in emulated["modules"]["audit_stages_cases"]["report"], emulated["modules"]["audit_stages_cases"]


def test_a_mixed_batch_forward_and_reversed(emulated):
    got = emulated["mixed_batch"]
    assert "error" not in got, got
    assert got["sizes"][1:3] == [140, 0] and got["stages"][0] > 0 and got["stages"][1:] == [0, 0, 0] and got["unscheduled"][3] > 0 and got["clean"] is True, got


def test_the_silent_edits_are_listed_under_pass_six_and_seven(emulated):
    got = emulated["silent_edits"]
    assert "error" not in got, got
    assert [e[1] for e in got["edits"]] == [6] * 4 + [7] * 9 and all(len(e[2]) == 1 for e in got["edits"]), got


def test_the_shapes_at_which_the_tail_can_go_wrong(emulated):
    got = emulated["tail_shapes"]
    assert "error" not in got, got
    assert [s[0] for s in got["shapes"]] == ["P = 1", "P = 257", "no pod relaxed at all", "M = 9"] and [s[1] for s in got["shapes"]][:3] == [1, 257, 3], got


def test_a_findings_cap_that_ends_inside_pass_six(emulated):
    got = emulated["cap"]
    assert "error" not in got, got
    assert got["counts"][1] == 2 and got["counts"][2] >= 1 and got["counts"][0] == got["counts"][1] + got["counts"][2], got
