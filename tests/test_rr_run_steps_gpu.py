"""(GPU) one STEP of ks_pack_rr's RUN rounds against the oracle, on the problems of tests/run_step_cases.py (tests/test_rr_run_steps.py runs the same
ones on the emulator): keys published side by side and one by one, the 8 / 9 boundary of a wave, two slots of one lane in one bucket and in one step, existing nodes
in front, hostname records inside a run, a commit that narrows a node's requirements, a run the exact filter stops."""
import pytest

import run_step_cases as RC
from karpenter_core_amd import scheduler as S
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(RC.CASES))
def test_run_steps_match_the_oracle(name, monkeypatch):
    monkeypatch.delenv("KS_NO_RR", raising=False)
    maker, shows = RC.CASES[name]
    p = maker()
    want = O.solve(p)
    if shows is not None:
        assert shows(want)
    fp = S.FlatProblem(p)
    try:
        got = fp.solve()
        started, why = fp.rr_status()
    finally:
        fp.close()
    assert started and why == 0, (started, why)         # ks_pack_rr took the Solve and kept it
    assert got.canonical() == want.canonical() and got.reasons == want.reasons
    assert got.stats.get("p22", 0) > 0, got.stats       # ... through RUN rounds
