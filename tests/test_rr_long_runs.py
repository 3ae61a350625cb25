"""(CPU) ks_pack_rr's RUN rounds over stretches longer than one 64-lane chunk of the queue (RR_RUN_MAX): the kernel's SOURCE on the lane-fibre emulator
(tests/simlib.py, in a subprocess like tests/test_rr_emulated.py) against the oracle -- placements, InstanceTypeOptions, stages and reasons -- on the problems of
tests/long_runs_cases.py: one stretch several tables long; stretches that end at and next to every chunk boundary and the cap; machines that fill up in the middle of a
chunk and at its boundary; hostname-keyed items that change inside a run; a requeued pod inside a later stretch; runs that start on existing nodes.  The problems
tests/test_rr_emulated.py reaches RUN rounds with (the config #3 shape at three sizes) and three committed seeds of the randomised families stay what they were."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import long_runs_cases as LC
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CHILD = r"""
import ctypes, hashlib, json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import long_runs_cases as LC, test_fuzz_mid as T, test_fuzz_rr as R
from karpenter_core_amd import workloads as W
lib = ctypes.CDLL(os.path.join(%(tests)r, "sim", "_build", "libksolve.so"))
lib.ks_rr_run_max.restype = ctypes.c_uint32
out = {"run_max": int(lib.ks_rr_run_max())}
def one(p):
    f = S.FlatProblem(p)
    try:
        r = f.solve(); st = f.rr_status()
    finally:
        f.close()
    return {"fp": hashlib.sha256(json.dumps(r.canonical(), sort_keys=True).encode()).hexdigest(),
            "reasons": hashlib.sha256(json.dumps(sorted((int(k), int(v)) for k, v in r.reasons.items())).encode()).hexdigest(),
            "rr": list(st), "run_pods": r.stats.get("p22", 0), "steps": r.stats.get("p23", 0), "runs": r.stats.get("p24", 0)}
CONFIG3 = json.loads(sys.argv[2])
for name in json.loads(sys.argv[1]):
    try:
        kind, _, seed = name.partition("_seed_")
        out[name] = one(R.rr_problem(int(seed)) if kind == "rr" else T.mid_problem(int(seed)) if kind == "mid" else W.config3(**CONFIG3[name]) if name in CONFIG3 else LC.CASES[name][0]())
    except Exception as e:
        out[name] = {"error": str(e)[:200]}
print("RESULT " + json.dumps(out))
"""

CONFIG3 = {"config3_140": {"pods": 140, "sizes": 3, "seed": 1}, "config3_700": {"pods": 700, "sizes": 10, "seed": 7}, "config3_3500": {"pods": 3500, "sizes": 20, "seed": 44}}
GOLDEN = ["rr_seed_9013", "mid_seed_0", "mid_seed_3"]


@pytest.fixture(scope="module")
def emulated():
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None); env.pop("KS_NO_RR", None)
    env["KS_SIM_ALARM"] = "600"
    code = CHILD % {"root": ROOT, "tests": HERE}
    pr = subprocess.run([sys.executable, "-c", code, json.dumps(list(LC.CASES) + GOLDEN + list(CONFIG3)), json.dumps(CONFIG3)], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, pr.stdout[-2000:] + pr.stderr[-2000:]
    return json.loads(line[-1][7:])


@pytest.mark.parametrize("name", list(LC.CASES))
def test_long_runs_match_the_oracle_on_the_emulator(emulated, name):
    got = emulated[name]
    assert "error" not in got, got
    assert got["rr"] == [1, 0], got                     # ks_pack_rr took the Solve and kept it
    want = O.solve(LC.CASES[name][0]())
    assert got["fp"] == hashlib.sha256(json.dumps(want.canonical(), sort_keys=True).encode()).hexdigest()
    assert got["reasons"] == hashlib.sha256(json.dumps(sorted((int(k), int(v)) for k, v in want.reasons.items())).encode()).hexdigest()
    assert got["run_pods"] > 0, got                     # ... through RUN rounds
    if LC.CASES[name][1] and emulated["run_max"] > 64:
        assert got["run_pods"] / got["runs"] > 64, got  # ... longer than one chunk of the queue


@pytest.mark.parametrize("name", GOLDEN)
def test_committed_seeds_stay_what_they_were(emulated, name):
    import test_fuzz_mid as T, test_fuzz_rr as R
    got = emulated[name]
    assert "error" not in got, got
    kind, _, seed = name.partition("_seed_")
    gold = (R._gold() if kind == "rr" else T._gold())[seed]
    assert (got["fp"], got["reasons"]) == (gold["sha256"], gold["reasons_sha256"])
    assert got["rr"] == [1, 0], got


@pytest.mark.parametrize("name", list(CONFIG3))
def test_the_config3_shape_stays_what_it_was(emulated, name):
    from karpenter_core_amd import workloads as W
    got = emulated[name]
    assert "error" not in got, got
    want = O.solve(W.config3(**CONFIG3[name]))
    assert got["fp"] == hashlib.sha256(json.dumps(want.canonical(), sort_keys=True).encode()).hexdigest()
    assert got["rr"] == [1, 0], got
    if name == "config3_3500":
        assert got["run_pods"] > 1000, got              # (the size at which the generic replicas come in stretches)


def test_the_run_cap_is_a_whole_number_of_chunks(emulated):
    assert emulated["run_max"] >= 64 and emulated["run_max"] % 64 == 0
