"""(CPU) ks_pack_rr at the last value each of its tables takes and at the first one past it: the kernel's SOURCE on the lane-fibre emulator (tests/simlib.py, in one
subprocess like tests/test_rr_long_runs.py) on the problems of tests/rr_limit_cases.py.  For every case: the result and the reasons are the oracle's, whichever
kernel ended up with the Solve; ks_pack_rr kept it or gave it back with exactly the code the catalogue names; and the same resident problem solved once more gives
the same (a decline in the middle of a run -- codes 2, 3, 4, 5, 7 -- leaves rr_memo, rr_mcnrc and the per-pod arrays written before ks_pack starts).  Per family:
the taken rungs are a prefix and both sides of the boundary are there; and the oracle's result alone says that the case stands where its name says it does.

The two node-count cases (thousands of one-pod machines: minutes for the oracle) compare with tests/golden/rr_limit_hashes.json and with the closed form."""
import json
import os
import subprocess
import sys

import pytest

import rr_limit_cases as RC
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHILD = r"""
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import rr_limit_cases as RC
out = {}
def one(name):
    p = RC.CASES[name][0]()
    f = S.FlatProblem(p)
    try:
        r = f.solve(); st = f.rr_status()
        again = f.solve(); st2 = f.rr_status()
        got = dict(RC.fingerprints(r), rr=[int(st[0]), int(st[1])], again=dict(RC.fingerprints(again), rr=[int(st2[0]), int(st2[1])]), dims=f.dims)
        if name in RC.GOLDEN:
            got["one_pod_each"] = RC.one_pod_each(r, len(p.pods))
        return got
    finally:
        f.close()
for name in RC.CASES:
    try:
        out[name] = one(name)
    except Exception as e:
        out[name] = {"error": str(e)[:300]}
try:
    S.FlatProblem(RC.UNSUPPORTED()).close()
    out["unsupported"] = "flattened"
except S.KSolveError as e:
    out["unsupported"] = [int(e.code), str(e)[:300]]
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def emulated():
    env = dict(os.environ)
    for k in ("KS_TEST_SIM", "KS_NO_RR", "KS_ONE_WAVE", "KS_NO_LEAN"):
        env.pop(k, None)
    env["KS_SIM_ALARM"] = "900"
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, pr.stdout[-2000:] + pr.stderr[-2000:]
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def oracle():
    """name -> (problem, the oracle's result), computed once per case and shared."""
    kept = {}

    def get(name):
        if name not in kept:
            p = RC.CASES[name][0]()
            kept[name] = (p, O.solve(p))
        return kept[name]
    return get


def _gold():
    return json.load(open(os.path.join(HERE, "golden", "rr_limit_hashes.json")))


@pytest.mark.parametrize("name", list(RC.CASES))
def test_limit_case_on_the_emulator(emulated, oracle, name):
    got = emulated[name]
    assert "error" not in got, got
    _, want_rr, _, _ = RC.CASES[name]
    if name in RC.GOLDEN:
        gold = _gold()[name]
        want = {"fp": gold["sha256"], "reasons": gold["reasons_sha256"]}
        assert gold["one_pod_each"] and gold["new_nodes"] == gold["pods"] == RC.CASES[name][3]
        assert got["one_pod_each"]                          # n nodes, node i holding queue entry i
    else:
        want = RC.fingerprints(oracle(name)[1])
    assert {k: got[k] for k in ("fp", "reasons")} == want   # the oracle's result and reasons, whichever kernel ended up with the Solve
    assert tuple(got["rr"]) == tuple(want_rr), got          # kept, or given back with exactly this code
    assert got["again"] == {"fp": got["fp"], "reasons": got["reasons"], "rr": got["rr"]}, got      # the resident problem once more


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_taken_rungs_are_a_prefix_and_both_sides_are_there(emulated, family):
    rungs = [(c[3], emulated[n].get("rr") == [1, 0]) for n, c in RC.CASES.items() if c[2] == family]
    assert RC.boundary_ok(family, rungs), rungs
    # ... and the catalogue itself says the same of what it expects
    assert RC.boundary_ok(family, [(c[3], tuple(c[1]) == RC.TAKEN) for c in RC.CASES.values() if c[2] == family])


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_the_cases_stand_where_they_say(emulated, oracle, family):
    """Not vacuous: read from the oracle's result (and the dimensions of the flat problem) alone -- the machine IS filled to 1 023 pods, the requirement records ARE
    k, G and GH ARE the rung, node index 448 IS there ..."""
    for name, (_, _, fam, rung) in RC.CASES.items():
        if fam != family:
            continue
        assert "error" not in emulated[name], emulated[name]
        if name in RC.GOLDEN:
            gold = _gold()[name]
            assert gold["new_nodes"] == rung and gold["one_pod_each"] and gold["unscheduled"] == 0, gold
        else:
            p, res = oracle(name)
            assert RC.STANDS[family](rung, p, res, emulated[name]["dims"]), (name, emulated[name]["dims"])


def test_every_family_has_its_check():
    assert set(RC.STANDS) | {"node_count"} == set(RC.FAMILIES)


def test_four_hostname_items_are_refused_by_the_flattening(emulated):
    """A pod with four hostname-keyed items never reaches a kernel (three is the class plan's room: the hostname_items family)."""
    assert emulated["unsupported"] != "flattened", "four hostname-keyed items were flattened"
    code, text = emulated["unsupported"]
    assert code == -2 and "hostname-keyed" in text, emulated["unsupported"]      # KS_ERR_UNSUPPORTED
