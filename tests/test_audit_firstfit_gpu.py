"""(GPU) The audit's fourth pass on the device (include/ksolve.h ks_audit_firstfit_dev, KS_AUDIT_POD_FIT_*; kernels in karpenter_core_amd/csrc/ks_audit_firstfit.inc)
against its literal reference (tests/audit_firstfit_ref.py):
  a) genuine results are clean and not vacuously so -- every flag zero, bit for bit what the reference says, `checked`, `admitting_pairs` and `skipped_pods` included --
     over the third pass's problem list (tests/audit_spread_cases.py GENUINE) with a few generic pods added, through ks_pack_rr and through ks_pack;
  b) a batch of what-ifs derived on the device against the same what-ifs flattened one by one;
  c) the tamper matrix through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  d) the shapes where the kernels take another path; the clauses of the new-node predicate in pairs; the same flags every run; the refusals.
tests/test_audit_firstfit.py runs the same kernels' source on the emulator."""
import pytest

import audit_firstfit_cases as FC
import audit_firstfit_ref as FR
import audit_harness as H
import audit_spread_cases as SC
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu

GENUINE = {name: (lambda make=make: FC.with_generic_pods(make())) for name, make in SC.GENUINE.items()}
CHECKED = {}      # (name, kernel) -> (pods examined, pairs, admitting pairs), filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name", list(GENUINE))
def test_genuine_results_are_clean(name, no_rr):
    f = S.FlatProblem(GENUINE[name](), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev = FC.assert_clean(S, f)
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} C {f.dims['C']} rr {f.rr_status()} {FC.summary(dev)} ms {dev['ms']}")
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == f.result_arrays()["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((f.result_arrays()["pod_node"] >= 0).sum())
        assert dev["checked"]["PODS"] >= 3      # the generic pods, at the least
        CHECKED[(name, no_rr)] = (dev["checked"]["PODS"], dev["checked"]["PAIRS"], dev["admitting_pairs"])
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    """Over the set the rule examined pods, evaluated (class, node) pairs and found some that admit."""
    got = {n: CHECKED[(n, no_rr)] for n in GENUINE if (n, no_rr) in CHECKED}
    assert len(got) == len(GENUINE), "runs after test_genuine_results_are_clean"
    print(got)
    assert all(v[0] > 0 and v[1] > 0 for v in got.values()) and sum(v[2] for v in got.values()) > 0, got


def test_a_batch_of_derived_whatifs_is_clean():
    """tests/audit_harness.py's decorated snapshot: the device pass over the batch derived on the device -- the snapshot's classes, the removed nodes skipped -- finds what
    the what-ifs flattened one by one say, nothing, over as many pods and pairs, as many of them admitting."""
    H.derived_whatifs_are_clean(FC.D, S, same=FC.summary, examined=lambda d: d["checked"]["PODS"])


@pytest.fixture(scope="module")
def matrix():
    return dict(FC.run_tamper_matrix(S))


@pytest.mark.parametrize("name", FC.TAMPER_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


@pytest.fixture(scope="module")
def shapes():
    return dict(FC.run_shapes(S))


@pytest.mark.parametrize("name", FC.SHAPE_NAMES)
def test_the_kernels_other_paths(shapes, name):
    """T = 1, 64, 65 and 130 with the only admitting type in the last bit; E = 0; n_new = 0; P = 1 with one used class; 257 used classes (the compaction crosses a scan
    tile); E = 65 and 257 with the only admitting node at index 0 and at E - 2 (the minimum crosses lanes, waves and workgroups); 1 100 pods on one node (the request
    sum); 12 resource names; two templates."""
    assert shapes[name] is True, shapes[name]


@pytest.fixture(scope="module")
def clauses():
    return dict(FC.run_clauses(S))


@pytest.mark.parametrize("name", FC.CLAUSE_NAMES)
def test_the_clauses_of_the_new_node_predicate(clauses, name):
    """Per clause a pair of claimed results that differ in that clause alone: the reference refuses the one and admits the other, and the kernels say what it says."""
    assert clauses[name] is True, clauses[name]


def test_flags_are_the_same_every_run():
    first = H.same_flags_every_run(FC.D, S, FC.tamper_problem(), lambda f: FC.tampers(f.result_arrays(), f.pod_seq(), FR.problem_arrays(S, f))[1][1:3])
    assert first["n_pods_flagged"] >= 1
    first = H.same_flags_every_run(FC.D, S, W.config3(pods=700, sizes=10, seed=7))      # new nodes and many classes: open[] and first_*[] by atomicMin, the sums by atomicAdd
    assert first["checked"]["PODS"] > 0


def test_refusals():
    H.refusals(FC.D, S, FC.tamper_problem())
