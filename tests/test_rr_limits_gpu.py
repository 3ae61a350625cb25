"""(GPU) ks_pack_rr at the last value each of its tables takes and at the first one past it, on the problems of tests/rr_limit_cases.py (tests/test_rr_limits.py runs
the same ones on the emulator, which only models the DPP, readlane and ballot operations the kernel is built from).  For every case: the result and the reasons
are the oracle's; ks_pack_rr kept the Solve or gave it back with exactly the code the catalogue names; the same resident problem solved once more gives the same; and
KS_FLAG_NO_RR on the same problem -- ks_pack from the start -- gives the oracle's result and reasons too.

The ladder family is the one whose boundary may differ from the emulator's: the kernel's dynamic LDS room is min(44 KiB, 160 KiB - its static LDS) here and a plain
44 KiB there.  Only its ends are pinned (600 distinct capacities taken, 1 900 given back) and that the taken rungs are a prefix."""
import json
import os

import pytest

import rr_limit_cases as RC
from karpenter_core_amd import scheduler as S
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LADDER_ENDS = {"ladders_600", "ladders_1900"}
_kept = {}


def _gold():
    return json.load(open(os.path.join(HERE, "golden", "rr_limit_hashes.json")))


def _case(name):
    """name -> everything the tests below read of one case, computed once: the problem, what the oracle says (its result, or the committed fingerprints of a
    node-count case), and the three Solves on the GPU (twice on one resident problem; once with KS_FLAG_NO_RR)."""
    if name in _kept:
        return _kept[name]
    saved = {k: os.environ.pop(k) for k in ("KS_NO_RR", "KS_ONE_WAVE", "KS_NO_LEAN") if k in os.environ}
    try:
        p = RC.CASES[name][0]()
        c = {"p": p}
        if name in RC.GOLDEN:
            gold = _gold()[name]
            c["want"], c["res"] = {"fp": gold["sha256"], "reasons": gold["reasons_sha256"]}, None
        else:
            c["res"] = O.solve(p)
            c["want"] = RC.fingerprints(c["res"])
        f = S.FlatProblem(p)
        try:
            r = f.solve(); c["rr"] = tuple(int(x) for x in f.rr_status())
            again = f.solve(); c["rr_again"] = tuple(int(x) for x in f.rr_status())
            c["got"], c["again"], c["dims"], c["one_pod_each"] = RC.fingerprints(r), RC.fingerprints(again), f.dims, RC.one_pod_each(r, len(p.pods))
        finally:
            f.close()
        f = S.FlatProblem(p, flags=S.KS_FLAG_NO_RR)
        try:
            alone = f.solve(); c["rr_alone"] = tuple(int(x) for x in f.rr_status())
            c["alone"] = RC.fingerprints(alone)
        finally:
            f.close()
    finally:
        os.environ.update(saved)
    _kept[name] = c
    return c


@pytest.mark.parametrize("name", list(RC.CASES))
def test_limit_case(name):
    c = _case(name)
    _, want_rr, family, rung = RC.CASES[name]
    print(f"{name}: rr_status {c['rr']} (emulator: {tuple(want_rr)}), again {c['rr_again']}, dims {c['dims']}")
    assert c["got"] == c["want"]                            # the oracle's result and reasons, whichever kernel ended up with the Solve
    if family != "ladders" or name in LADDER_ENDS:
        assert c["rr"] == tuple(want_rr), c["rr"]           # kept, or given back with exactly this code
    else:
        assert c["rr"] in ((1, 0), (1, 1)), c["rr"]         # (between the ends the LDS room decides)
    assert c["again"] == c["got"] and c["rr_again"] == c["rr"]      # the resident problem once more
    assert c["rr_alone"][0] == 0 and c["alone"] == c["want"]        # ks_pack from the start (KS_FLAG_NO_RR travels with the problem)
    if name in RC.GOLDEN:
        assert c["one_pod_each"]                            # n nodes, node i holding queue entry i


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_taken_rungs_are_a_prefix_and_both_sides_are_there(family):
    rungs = [(c[3], _case(n)["rr"] == RC.TAKEN) for n, c in RC.CASES.items() if c[2] == family]
    assert RC.boundary_ok(family, rungs), rungs


@pytest.mark.parametrize("family", RC.FAMILIES)
def test_the_cases_stand_where_they_say(family):
    """Not vacuous: read from the oracle's result (and the dimensions of the flat problem) alone."""
    for name, (_, _, fam, rung) in RC.CASES.items():
        if fam != family:
            continue
        if name in RC.GOLDEN:
            gold = _gold()[name]
            assert gold["new_nodes"] == rung and gold["one_pod_each"] and gold["unscheduled"] == 0, gold
        else:
            c = _case(name)
            assert RC.STANDS[family](rung, c["p"], c["res"], c["dims"]), (name, c["dims"])


def test_four_hostname_items_are_refused_by_the_flattening():
    with pytest.raises(S.KSolveError, match="hostname-keyed") as e:
        S.FlatProblem(RC.UNSUPPORTED()).close()
    assert e.value.code == S.KS_ERR_UNSUPPORTED
