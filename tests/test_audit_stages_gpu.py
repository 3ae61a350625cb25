"""(GPU) The audit's seventh pass on the device (include/ksolve.h ks_audit_stages_dev, KS_AUDIT_POD_STAGE_*; kernels in karpenter_core_amd/csrc/ks_audit_stages.inc and
four of the fourth pass's) against its literal reference (tests/audit_stages_ref.py) -- device flags and every counter compared with the reference, not the emulator:
  a) the family of problems in which pods relax (tests/audit_stages_cases.py) is clean and not vacuously so, through ks_pack_rr and through ks_pack;
  b) a batch of what-ifs with removed nodes derived on the device against the same what-ifs flattened one by one;
  c) the tamper matrix through the claimed form, the commit numbers read from ksh_placement_rows and edited, through both pack kernels;
  d) the shapes where the kernels take another path, through both pack kernels; the same flags every run; the refusals.
tests/test_audit_stages.py runs the same kernels' source on the emulator."""
import numpy as np
import pytest

import audit_harness as H
import audit_stages_cases as SC
from karpenter_core_amd import scheduler as S

pytestmark = pytest.mark.gpu

CHECKED = {}      # (name, kernel) -> the reference's counts, filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name,args", SC.FAMILY, ids=[n for n, _ in SC.FAMILY])
def test_the_family_is_clean(name, args, no_rr):
    f = S.FlatProblem(SC.relax_problem(**args), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev, ref = SC.compare(S, f)
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} C {f.dims['C']} rr {f.rr_status()} {SC.summary_with_reference(dev, ref)} ms {dev['ms']}")
        assert not dev["pod_flags"].any() and dev["n_pods_flagged"] == 0, dev["pod_bit_count"]
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == f.result_arrays()["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((f.result_arrays()["pod_node"] >= 0).sum())
        CHECKED[(name, no_rr)] = (dev["checked"]["PODS"], dev["checked"]["STAGES"], ref["pairs_existing"], ref["pairs_template"], ref["unscheduled_examined"])
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    """Over the family: examined pods, examined stages, existing-node pairs, template pairs, unscheduled pods with an examined earlier stage -- none of them zero."""
    got = [CHECKED[(n, no_rr)] for n, _ in SC.FAMILY if (n, no_rr) in CHECKED]
    assert len(got) == len(SC.FAMILY), "runs after test_the_family_is_clean"
    sums = [sum(v[i] for v in got) for i in range(5)]
    print(sums)
    assert all(x > 0 for x in sums), sums


def test_a_batch_of_derived_whatifs_is_clean():
    """tests/audit_stages_cases.py's snapshot, whose bound pods carry preferences nothing satisfies, with nodes removed: the device pass over the batch derived on the
    device -- the snapshot's classes, the removed nodes skipped -- counts what the what-ifs flattened one by one count, and finds nothing."""
    plain, derived = SC.derived_whatifs(S)
    print(plain)


KERNELS = {"ks_pack_rr": 0, "ks_pack": S.KS_FLAG_NO_RR}
_RAN = {}


def _once(what, run, kernel):
    if (what, kernel) not in _RAN:
        _RAN[(what, kernel)] = dict(run(S, KERNELS[kernel]))
    return _RAN[(what, kernel)]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", SC.TAMPER_NAMES)
def test_tamper_matrix(name, kernel):
    got = _once("tamper", SC.run_tamper_matrix, kernel)
    assert got[name] is True, (name, got[name])


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("name", SC.SHAPE_NAMES)
def test_the_kernels_other_paths(name, kernel):
    got = _once("shapes", SC.run_shapes, kernel)
    assert got[name] is True, (name, got[name])


def test_three_runs_raise_the_same_flags():
    """The resident form over the largest member of the family, and the claimed form over an edit that flags: byte-identical flags and the same counts, three times."""
    first = H.same_flags_every_run(SC.D, S, SC.relax_problem(3, True))
    assert not first["pod_flags"].any() and first["checked"]["STAGES"] > 0

    def claim(flat):
        res, seq = H._claimable(flat.result_arrays()), np.array(flat.pod_seq(), dtype=np.int32)
        res["pod_stage"][SC.PODS.index("team_a")] = 1
        res["pod_stage"][SC.PODS.index("zonal_a")] = 1
        res["pod_stage"][SC.PODS.index("giant")] = 0
        return res, seq
    first = H.same_flags_every_run(SC.D, S, SC.tamper_problem(), claim)
    assert H.flagged(first["pod_flags"]) == {SC.PODS.index("team_a"): SC.B["STAGE_EXISTING"], SC.PODS.index("zonal_a"): SC.B["STAGE_TEMPLATE"], SC.PODS.index("giant"): SC.B["STAGE_UNRELAXED"]}


def test_refusals():
    H.refusals(SC.D, S, SC.many_relaxed(2), totals=lambda o, f: o.checked[1] == 1 and o.checked[2] == 1 and o.checked[3] == 3 and o.skipped_pods == 1 and o.admitting_pairs == 0)
