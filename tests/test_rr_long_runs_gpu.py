"""(GPU) ks_pack_rr's RUN rounds over stretches longer than one 64-lane chunk of the queue (RR_RUN_MAX) against the oracle, on the problems of
tests/long_runs_cases.py (tests/test_rr_long_runs.py runs the same ones on the emulator), and once more through ks_pack (KS_NO_RR=1) -- the kernel a decline
would hand them to.  Three committed seeds of the randomised families stay what they were (the config #3 shape at the sizes that reach RUN rounds is
tests/test_rr_gpu.py's)."""
import ctypes
import os

import pytest

import long_runs_cases as LC
from karpenter_core_amd import scheduler as S
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


def _run_max():
    lib = ctypes.CDLL(os.path.join(os.path.dirname(S.__file__), "libksolve.so"))
    lib.ks_rr_run_max.restype = ctypes.c_uint32
    return int(lib.ks_rr_run_max())


def _solve(p, flags=0):
    fp = S.FlatProblem(p, flags=flags)
    try:
        res = fp.solve()
        return res, fp.rr_status()
    finally:
        fp.close()


@pytest.mark.parametrize("name", list(LC.CASES))
def test_long_runs_match_the_oracle(name, monkeypatch):
    monkeypatch.delenv("KS_NO_RR", raising=False)
    maker, long_ = LC.CASES[name]
    p = maker()
    want = O.solve(p)
    got, (started, why) = _solve(p)
    assert started and why == 0, (started, why)         # ks_pack_rr took the Solve and kept it
    assert got.canonical() == want.canonical() and got.reasons == want.reasons
    runs, run_pods = got.stats.get("p24", 0), got.stats.get("p22", 0)
    assert run_pods > 0, got.stats                      # ... through RUN rounds
    if long_ and _run_max() > 64:
        assert run_pods / runs > 64, (run_pods, runs)   # ... longer than one chunk of the queue
    monkeypatch.setenv("KS_NO_RR", "1")
    alone, (started2, _) = _solve(p)
    assert not started2
    assert alone.canonical() == want.canonical() and alone.reasons == want.reasons


@pytest.mark.parametrize("kind,seed", [("rr", 9013), ("mid", 0), ("mid", 3)])
def test_committed_seeds_stay_what_they_were(kind, seed, monkeypatch):
    import test_fuzz_mid as T, test_fuzz_rr as R
    monkeypatch.delenv("KS_NO_RR", raising=False)
    p, gold, fps = (R.rr_problem(seed), R._gold()[str(seed)], R.fingerprints) if kind == "rr" else (T.mid_problem(seed), T._gold()[str(seed)], T.fingerprints)
    got, (started, why) = _solve(p)
    assert started and why == 0, (started, why)
    assert fps(got) == {"sha256": gold["sha256"], "reasons_sha256": gold["reasons_sha256"]}
