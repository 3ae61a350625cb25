"""(GPU) The audit's eighth pass on the device (include/ksolve.h ks_audit_reasons_dev, KS_AUDIT_POD_REASON_*; kernels in karpenter_core_amd/csrc/ks_audit_reasons.inc
and the fourth pass's compaction) against its literal reference (tests/audit_reasons_ref.py) -- device flags and every counter compared with the reference, not the
emulator:
  a) the family of problems in which pods stay unscheduled (tests/audit_reasons_cases.py) is clean and not vacuously so, through ks_pack_rr and through ks_pack;
  b) the tamper matrix through the claimed form, through both pack kernels;
  c) the shapes where the kernels take another path, through both pack kernels: T = 1, 64, 65 and 130 with the only admitting type in the last bit, M = 1, 8 and 9,
     P = 1, 2 * 256 + 1 pods, 257 used classes, a class naming the last key, E = 0, a result with no unscheduled pod;
  d) a batch of three problems of different sizes; what-ifs derived on the device; the same tables every run; the refusals.
tests/test_audit_reasons.py runs the same kernels' source on the emulator."""
import numpy as np
import pytest

import audit_harness as H
import audit_reasons_cases as RC
import audit_topo_cases as TC
from karpenter_core_amd import scheduler as S

pytestmark = pytest.mark.gpu

CHECKED = {}      # (name, kernel) -> the device's counts, filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name,args", RC.FAMILY, ids=[n for n, _ in RC.FAMILY])
def test_the_family_is_clean(name, args, no_rr):
    f = S.FlatProblem(RC.stay_problem(**args), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev, ref = RC.compare(S, f)
        res = f.result_arrays()
        t = RC.tally(dev, ref, res, RC.RR.problem_arrays(S, f))
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} C {f.dims['C']} M {f.dims['M']} rr {f.rr_status()} {t} ms {dev['ms']}")
        assert not dev["pod_flags"].any() and dev["n_pods_flagged"] == 0, dev["pod_bit_count"]
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == res["n_new"]
        assert dev["n_placed"] == int((res["pod_node"] >= 0).sum()) and dev["n_unscheduled"] == len(res["unscheduled"]) == dev["checked"]["PODS"] > 0
        assert all(no == 0 for _, no in t["exact"].values()), t["exact"]
        CHECKED[(name, no_rr)] = [dev["checked"][k] for k in RC.RR.CHECKED]
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    """Over the family: unscheduled pods examined, nibbles decided exactly, bounded and not examined -- none of them zero."""
    got = [CHECKED[(n, no_rr)] for n, _ in RC.FAMILY if (n, no_rr) in CHECKED]
    assert len(got) == len(RC.FAMILY), "runs after test_the_family_is_clean"
    sums = [sum(v[i] for v in got) for i in range(4)]
    print(sums)
    assert all(x > 0 for x in sums), sums


KERNELS = {"ks_pack_rr": 0, "ks_pack": S.KS_FLAG_NO_RR}
_RAN = {}


def _once(what, run, kernel):
    if (what, kernel) not in _RAN:
        _RAN[(what, kernel)] = dict(run(S, KERNELS[kernel]))
    return _RAN[(what, kernel)]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", RC.TAMPER_NAMES)
def test_tamper_matrix(name, kernel):
    got = _once("tamper", RC.run_tamper_matrix, kernel)
    assert got[name] is True, (name, got[name])


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", RC.SHAPE_NAMES)
def test_the_kernels_other_paths(name, kernel):
    got = _once("shapes", RC.run_shapes, kernel)
    assert got[name] is True, (name, got[name])


def test_a_batch_of_three_problems_of_different_sizes():
    """One call over three results of different P, C, M and E says what one call each says -- flags and every counter --, and each agrees with the reference."""
    problems = [RC.stay_problem(**RC.FAMILY[3][1]), RC.many_pods(513), TC.plain(3, True)]
    flats = [S.FlatProblem(p) for p in problems]
    try:
        for f in flats:
            f.solve(decode=False)
        alone =[RC.compare(S, f)[0] for f in flats]
        batch = S.audit_reasons_batch(flats)
        assert len({(f.dims["P"], f.dims["M"], f.dims["E"]) for f in flats}) == 3
        for a, b in zip(alone, batch):
            assert np.array_equal(a["pod_flags"], b["pod_flags"]) and RC.summary(a) == RC.summary(b), (RC.summary(a), RC.summary(b))
        assert [b["checked"]["PODS"] > 0 for b in batch] == [True, True, False]
    finally:
        for f in flats:
            f.close()


def test_a_batch_of_derived_whatifs_is_clean():
    """tests/test_whatif_derived.py's decorated snapshot with nodes removed: the device pass over the batch derived on the device -- the snapshot's classes, the
    removed nodes' pods naming no node -- counts what the what-ifs flattened one by one count, and finds nothing."""
    keys = ("checked", "skipped_pods", "n_unscheduled", "used_classes", "pairs", "n_new", "n_placed")
    H.derived_whatifs_are_clean(RC.D, S, same=lambda d: [d[k] for k in keys], examined=lambda d: d["n_placed"])


def test_two_runs_of_one_call_give_identical_tables():
    """The resident form over the largest member of the family, and the claimed form over edits that flag: byte-identical flags and the same counts every run."""
    first = H.same_flags_every_run(RC.D, S, RC.stay_problem(**RC.FAMILY[6][1]))
    assert not first["pod_flags"].any() and first["checked"]["EXACT"] > 0 and first["checked"]["BOUNDED"] > 0 and first["checked"]["UNEXAMINED"] > 0
    pr = RC.tamper_problem()
    want = {}

    def claim(flat):
        res = flat.result_arrays()
        edits = RC.tampers(res, [p.uid for p in pr.pods])
        claimed = H._claimable(res)
        claimed["pod_reason"] = np.array(claimed["pod_reason"], dtype=np.uint32)
        for i in (0, 2, 4):      # a placed pod given a word, 2 and 4 swapped, 5 become 4: three different pods
            (p, bits), = edits[i][2].items()
            claimed["pod_reason"][p] = edits[i][1]["pod_reason"][p]
            want[p] = bits
        return (claimed,)
    first = H.same_flags_every_run(RC.D, S, pr, claim)
    assert H.flagged(first["pod_flags"]) == want and len(want) == 3


def test_refusals():
    H.refusals(RC.D, S, RC.many_pods(4, 1), totals=lambda o, f: o.checked[0] == 1 and o.checked[1] == 1 and o.n_placed == 3 and o.n_unscheduled == 1 and o.skipped_pods == 0 and o.pairs == 1)
