"""(GPU) The audit's ninth pass on the device (include/ksolve.h ks_audit_zonefit_dev, KS_AUDIT_POD_ZFIT_*; kernels in karpenter_core_amd/csrc/ks_audit_zonefit.inc)
against its literal reference (tests/audit_zonefit_ref.py):
  a) genuine results are clean -- every flag zero, bit for bit what the reference says, every counter included -- over the `zonal_cluster` seeds, through ks_pack_rr
     and through ks_pack, and not vacuously so;
  b) a batch of what-ifs derived on the device against the same what-ifs flattened one by one;
  c) the tamper matrix and the claimed results with indices out of range (proved on the emulator first: tests/test_audit_zonefit.py) through the claimed form;
  d) the shapes where the kernels take another path, the three runs with identical bytes and the slice switch among them.
tests/test_audit_zonefit.py runs the same kernels' source on the emulator; the refusals are tests/test_audit_zonefit_refusals.py's."""
import pytest

import audit_harness as H
import audit_zonefit_cases as ZC
from karpenter_core_amd import scheduler as S

pytestmark = pytest.mark.gpu
CHECKED = {}      # (seed, kernel) -> (pods examined, pairs, passed the zone test, admitting pairs, exact pods), filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("seed", ZC.SEEDS)
def test_genuine_results_are_clean(seed, no_rr):
    f = S.FlatProblem(ZC.zonal_cluster(seed), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev = ZC.assert_clean(S, f)
        print(f"seed {seed}: P {f.dims['P']} E {f.dims['E']} C {f.dims['C']} G {f.dims['G']} rr {f.rr_status()} {ZC.summary(dev)} ms {dev['ms']}")
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == f.result_arrays()["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((f.result_arrays()["pod_node"] >= 0).sum())
        assert dev["eligible_groups"] + dev["skipped_groups"] == f.dims["G"]
        CHECKED[(seed, no_rr)] = (dev["checked"]["PODS"], dev["checked"]["ZONE"], dev["checked"]["STATIC"], dev["admitting_pairs"], dev["exact_pods"])
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    got = {n: CHECKED[(n, no_rr)] for n in ZC.SEEDS if (n, no_rr) in CHECKED}
    assert len(got) == len(ZC.SEEDS), "runs after test_genuine_results_are_clean"
    print(got)
    assert all(min(v) > 0 and v[1] >= v[2] >= v[3] for v in got.values()), got


def test_a_batch_of_derived_whatifs_is_clean():
    """tests/audit_harness.py's decorated snapshot: the device pass over the batch derived on the device finds what the what-ifs flattened one by one say, nothing, over
    as many pods and pairs; a claimed result on a derived view is KS_ERR_UNSUPPORTED."""
    H.derived_whatifs_are_clean(ZC.D, S, same=lambda d: dict(ZC.summary(d), groups=d["eligible_groups"]), examined=lambda d: d["checked"]["PODS"])


@pytest.fixture(scope="module")
def matrix():
    return dict(ZC.run_tamper_matrix(S))


@pytest.mark.parametrize("name", ZC.TAMPER_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


@pytest.fixture(scope="module")
def ranges():
    return dict(ZC.run_range_cases(S))


@pytest.mark.parametrize("name", ZC.RANGE_NAMES)
def test_claimed_indices_out_of_range(ranges, name):
    """Flags or skips, never an access past a table: every index is range-checked before it addresses memory (the same cases pass on the emulator, where an access
    past a table is a host fault, in tests/test_audit_zonefit.py)."""
    assert ranges[name] is True, ranges[name]


@pytest.fixture(scope="module")
def clauses():
    return dict(ZC.run_clauses(S))


@pytest.mark.parametrize("name", ZC.CLAUSE_NAMES)
def test_the_clauses_of_the_new_node_predicate(clauses, name):
    """The Fits pair and the taint pair of tests/audit_firstfit_cases.py through this pass's kernels: the reference refuses the one and admits the other, and the kernels
    say what it says."""
    assert clauses[name] is True, clauses[name]


@pytest.fixture(scope="module")
def shapes():
    return dict(ZC.run_shapes(S))


@pytest.mark.parametrize("name", ZC.SHAPE_NAMES)
def test_the_kernels_other_paths(shapes, name):
    """2 x 256 + 65 pods with the offender just behind a tile and a chunk boundary; a key of 64 values with the only admissible one at value 63; two groups on two keys
    with the refusal in the second; a class at KS_AZ_GROUPS groups and one above it; E = 0; n_new = 0; P = 1; no eligible group (the early-out); E = 65 and 257 with the
    only admitting node at index 0 and at E - 2; T = 65 with the only admitting type in the last bit; three runs with identical bytes; one problem per slice."""
    assert shapes[name] is True, shapes[name]
