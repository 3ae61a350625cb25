"""(GPU) The audit's third pass on the device (include/ksolve.h ks_audit_spread_dev, KS_AUDIT_POD_SPREAD; kernels in karpenter_core_amd/csrc/ks_audit_spread.inc)
against its literal reference (tests/audit_spread_ref.py):
  a) genuine results are clean and not vacuously so -- every flag zero, bit for bit what the reference says, `checked` and `exact_pairs` included -- over the
     topology-bearing problems of tests/test_audit_topology_gpu.py's list and the zonal spreads of tests/audit_spread_cases.py, through ks_pack_rr and through ks_pack;
  b) a batch of what-ifs derived on the device against the same what-ifs flattened one by one;
  c) the tamper matrix through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_spread.py runs the same kernels' source on the emulator."""
import pytest

import audit_harness as H
import audit_spread_cases as SC
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu

GENUINE = SC.GENUINE
CHECKED = {}      # (name, kernel) -> (pairs, exact pairs), filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name", list(GENUINE))
def test_genuine_results_are_clean(name, no_rr):
    f = S.FlatProblem(GENUINE[name](), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev = SC.assert_clean(S, f)
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} G {f.dims['G']} rr {f.rr_status()} {SC.summary(dev)} ms {dev['ms']}")
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == f.result_arrays()["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((f.result_arrays()["pod_node"] >= 0).sum())
        CHECKED[(name, no_rr)] = (dev["checked"]["SPREAD"], dev["exact_pairs"])
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    """Over the set the rule examined pairs, the generators' problems among them, and some of them exactly."""
    got = {n: CHECKED[(n, no_rr)] for n in GENUINE if (n, no_rr) in CHECKED}
    assert len(got) == len(GENUINE), "runs after test_genuine_results_are_clean"
    print(got)
    generators = [v for n, v in got.items() if n not in ("a zonal spread on labelled nodes", "two keys")]
    assert sum(v[0] for v in generators) > 100 and sum(v[1] for v in got.values()) > 0, got
    assert got["a zonal spread on labelled nodes"] == (40, 40) and got["two keys"] == (8, 8)


def test_a_batch_of_derived_whatifs_is_clean():
    """tests/audit_harness.py's decorated snapshot: the device pass over the batch derived on the device finds what the what-ifs flattened one by one say -- nothing --
    over as many placed pods and pairs, as many of them exact."""
    def sliced(derived, got):
        assert SC.sliced_batch_says_the_same(S, derived, got)
    H.derived_whatifs_are_clean(SC.D, S, same=lambda d: (d["n_new"], d["n_placed"], d["checked"], d["exact_pairs"]), examined=lambda d: d["checked"]["SPREAD"], after=sliced)


@pytest.fixture(scope="module")
def matrix():
    return dict(SC.run_tamper_matrix(S))


@pytest.mark.parametrize("name", SC.TAMPER_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


@pytest.fixture(scope="module")
def shapes():
    return dict(SC.run_shapes(S))


@pytest.mark.parametrize("name", SC.SHAPE_NAMES)
def test_the_kernels_other_paths(shapes, name):
    """2 * 256 + 65 pods across two chunk boundaries and a tile boundary, one late pod claimed into the fullest zone; a key of 64 values with the violation in value id
    63; two groups on two keys with the violation in the second; P = 1; G = 0 with n_new = 0; a problem whose only spread is over the hostname."""
    assert shapes[name] is True, shapes[name]


def test_flags_are_the_same_every_run():
    first = H.same_flags_every_run(SC.D, S, SC.tamper_problem(), lambda f: SC.tampers(f.result_arrays(), f.pod_seq())[1][1:3])
    assert first["n_pods_flagged"] == 2
    first = H.same_flags_every_run(SC.D, S, W.config3(pods=700, sizes=10, seed=7))      # new nodes: the pin table is built with atomicMin, the chunk table with atomicAdd
    assert first["checked"]["SPREAD"] > 0


def test_refusals():
    H.refusals(SC.D, S, SC.tamper_problem())
