"""(GPU) The audit's sixth pass on the device (include/ksolve.h ks_audit_hostfit_dev, KS_AUDIT_POD_HFIT_*; kernels in karpenter_core_amd/csrc/ks_audit_hostfit.inc)
against its literal reference (tests/audit_hostfit_ref.py):
  a) genuine results are clean -- every flag zero, bit for bit what the reference says, every counter included -- over the problem list of
     tests/audit_spread_cases.py (GENUINE) with a few hostname-spread pods added, through ks_pack_rr and through ks_pack, and not vacuously so;
  b) rr_problem(9013): the fourth pass examines no pod of it, this pass examines pod 810, and the historical edit raises HFIT_NEW;
  c) a batch of what-ifs derived on the device -- removed nodes among them -- against the same what-ifs flattened one by one;
  d) the tamper matrix and the claimed results with indices out of range (proved on the emulator first: tests/test_audit_hostfit.py) through the claimed form;
  e) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_hostfit.py runs the same kernels' source on the emulator."""
import copy

import pytest

import audit_harness as H
import audit_hostfit_cases as HC
import audit_spread_cases as SC
import audit_topo_cases as TC
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu


def _with_spread_pods(pr, n=3):
    """`pr` with a few pods under a hostname spread of their own at the end of its list: whatever else the problem holds, some pod of it is examined."""
    pr = copy.copy(pr)
    pr.pods = list(pr.pods) + [TC._pod("zz-hostfit-%d" % i, app="zz-hostfit", cpu="10m", mem="8Mi", spread=HC._spread(1, "zz-hostfit")) for i in range(n)]
    return pr


GENUINE = {name: (lambda make=make: _with_spread_pods(make())) for name, make in SC.GENUINE.items()}
CHECKED = {}      # (name, kernel) -> (pods examined, pairs, count tests, admitting pairs), filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name", list(GENUINE))
def test_genuine_results_are_clean(name, no_rr):
    f = S.FlatProblem(GENUINE[name](), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev = HC.assert_clean(S, f)
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} C {f.dims['C']} G {f.dims['G']} rr {f.rr_status()} {HC.summary(dev)} ms {dev['ms']}")
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == f.result_arrays()["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((f.result_arrays()["pod_node"] >= 0).sum())
        assert dev["checked"]["PODS"] >= 3 and dev["eligible_groups"] >= 1      # the added pods, at the least
        assert dev["eligible_groups"] + dev["skipped_groups"] == f.dims["G"]
        CHECKED[(name, no_rr)] = (dev["checked"]["PODS"], dev["checked"]["PAIRS"], dev["checked"]["TESTS"], dev["admitting_pairs"])
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    got = {n: CHECKED[(n, no_rr)] for n in GENUINE if (n, no_rr) in CHECKED}
    assert len(got) == len(GENUINE), "runs after test_genuine_results_are_clean"
    print(got)
    assert all(v[0] > 0 and v[1] > 0 and v[2] >= v[1] for v in got.values()) and sum(v[3] for v in got.values()) > 0, got


def test_rr_9013_is_examined_and_the_historical_edit_is_flagged():
    """The problem whose parity bug the randomised net caught: the fourth pass examines none of its pods, this pass examines pod 810 -- and with
    pod 810 claimed as the opener of an added node while the node it joined has room again, it raises HFIT_NEW on it."""
    import test_fuzz_rr as R
    f = S.FlatProblem(R.rr_problem(9013))
    try:
        f.solve(decode=False)
        dev = HC.assert_clean(S, f)
        print(HC.summary(dev), dev["ms"])
        assert f.audit_firstfit()["checked"]["PODS"] == 0 and dev["checked"]["PODS"] > 0 and dev["checked"]["TESTS"] > 0 and dev["admitting_pairs"] > 0
        h = HC.historical_case(S, f)
        print(h)
        assert h["pod_810_examined"] is True and h["ok"] is True and h["pod"] == HC.HISTORICAL_POD and h["flags"] == HC.B["HFIT_NEW"], h
    finally:
        f.close()


def test_a_batch_of_derived_whatifs_with_removed_nodes_is_clean():
    """tests/audit_harness.py's decorated snapshot: the device pass over the batch derived on the device -- the snapshot's classes and groups, the removed nodes skipped
    and their hostnames unregistered (init == -1) -- finds what the what-ifs flattened one by one say, nothing, over as many pods, pairs and count tests, as many of them
    admitting.  (A derived what-if numbers the snapshot's groups: more of them are skipped, as many are eligible.)"""
    H.derived_whatifs_are_clean(HC.D, S, same=lambda d: dict(HC.summary(d), groups=d["eligible_groups"]), examined=lambda d: d["checked"]["PODS"])


@pytest.fixture(scope="module")
def matrix():
    return dict(HC.run_tamper_matrix(S))


@pytest.mark.parametrize("name", HC.TAMPER_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


@pytest.fixture(scope="module")
def ranges():
    return dict(HC.run_range_cases(S))


@pytest.mark.parametrize("name", HC.RANGE_NAMES)
def test_claimed_indices_out_of_range(ranges, name):
    """Flags or skips, never an access past a table: every index is range-checked before it addresses memory (the same cases pass on the emulator, where an access
    past a table is a host fault, in tests/test_audit_hostfit.py)."""
    assert ranges[name] is True, ranges[name]


@pytest.fixture(scope="module")
def clauses():
    return dict(HC.run_clauses(S))


@pytest.mark.parametrize("name", HC.CLAUSE_NAMES)
def test_the_clauses_of_the_new_node_predicate(clauses, name):
    """The Fits pair and the taint pair of tests/audit_firstfit_cases.py through this pass's kernels: the reference refuses the one and admits the other, and the kernels
    say what it says."""
    assert clauses[name] is True, clauses[name]


@pytest.fixture(scope="module")
def shapes():
    return dict(HC.run_shapes(S))


@pytest.mark.parametrize("name", HC.SHAPE_NAMES)
def test_the_kernels_other_paths(shapes, name):
    """1, 64 and 65 eligible groups; a class under the most groups a problem may hold; E = 0; n_new = 0; P = 1; E = 65 and 257 with the only admitting node -- by its
    count alone -- at index 0 and at E - 2; 65 new nodes of which only the first-opened admits; T = 1 and 65 with the only admitting type in the last bit; maxSkew 1 and
    2, self and not, at the boundary and one past it; init 0 and 1 (-1: the derived batch above); 257 used classes; 1 100 pods on one node; 12 resource names; two
    templates."""
    assert shapes[name] is True, shapes[name]


def test_flags_are_the_same_every_run():
    first = H.same_flags_every_run(HC.D, S, HC.tamper_problem(), lambda f: HC.tampers(f.result_arrays(), f.pod_seq())[1][1:3])
    assert first["n_pods_flagged"] >= 1
    first = H.same_flags_every_run(HC.D, S, W.hostname_herd(pods=600, labels=3, seed=3))      # new nodes, many pods per group: fin by atomicAdd, open[] and first_*[] by atomicMin
    assert first["checked"]["PODS"] > 0


def test_refusals():
    H.refusals(HC.D, S, HC.tamper_problem())
