"""(CPU) one STEP of ks_pack_rr's RUN rounds: what a wave publishes -- every accepting key of the bucket side by side when it holds at most eight, its
eight smallest one by one when it holds more or an existing node leads -- the flag on an eighth key, and the commit of a slot's winners side by side.  The kernel's
SOURCE on the lane-fibre emulator (tests/simlib.py, in a subprocess like tests/test_rr_long_runs.py) against the oracle -- placements, InstanceTypeOptions, stages
and reasons -- on the problems of tests/run_step_cases.py.  (The emulator build checks the census of zero hostname counters itself.)"""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import run_step_cases as RC
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHILD = r"""
import hashlib, json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import run_step_cases as RC
out = {}
def one(p):
    f = S.FlatProblem(p)
    try:
        r = f.solve(); st = f.rr_status()
    finally:
        f.close()
    return {"fp": hashlib.sha256(json.dumps(r.canonical(), sort_keys=True).encode()).hexdigest(),
            "reasons": hashlib.sha256(json.dumps(sorted((int(k), int(v)) for k, v in r.reasons.items())).encode()).hexdigest(),
            "rr": list(st), "run_pods": r.stats.get("p22", 0), "steps": r.stats.get("p23", 0), "runs": r.stats.get("p24", 0), "exact": r.stats.get("cyc_stage", 0)}
for name in json.loads(sys.argv[1]):
    try:
        out[name] = one(RC.CASES[name][0]())
    except Exception as e:
        out[name] = {"error": str(e)[:200]}
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def emulated():
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None); env.pop("KS_NO_RR", None)
    env["KS_SIM_ALARM"] = "600"
    code = CHILD % {"root": ROOT, "tests": HERE}
    pr = subprocess.run([sys.executable, "-c", code, json.dumps(list(RC.CASES))], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, pr.stdout[-2000:] + pr.stderr[-2000:]
    return json.loads(line[-1][7:])


@pytest.mark.parametrize("name", list(RC.CASES))
def test_run_steps_match_the_oracle_on_the_emulator(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["rr"] == [1, 0], got                     # ks_pack_rr took the Solve and kept it
    maker, shows = RC.CASES[name]
    want = O.solve(maker())
    if shows is not None:
        assert shows(want)                              # the oracle's placements are the ones the case is about
    assert got["fp"] == hashlib.sha256(json.dumps(want.canonical(), sort_keys=True).encode()).hexdigest()
    assert got["reasons"] == hashlib.sha256(json.dumps(sorted((int(k), int(v)) for k, v in want.reasons.items())).encode()).hexdigest()
    assert got["run_pods"] > 0, got                     # ... through RUN rounds


def test_the_exact_filter_stops_a_run(emulated):
    got = emulated["narrowing_changes_the_capacity"]
    assert got["exact"] > 0 and got["run_pods"] > 0, got      # (exact checks: statistics slot 13 of a build without probes)
    assert emulated["zone_selector_on_open_machines"]["exact"] == 0
