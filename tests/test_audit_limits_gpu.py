"""(GPU) The audit's fifth pass on the device (include/ksolve.h ks_audit_limits_dev, KS_AUDIT_NODE_LIMIT_*, KS_AUDIT_POD_LIMIT_TEMPLATE; kernels in
karpenter_core_amd/csrc/ks_audit_limits.inc) against its literal reference (tests/audit_limits_ref.py):
  a) the genuine problems are clean -- every flag zero, bit for bit what the reference says, every counter included -- through ks_pack (ks_pack_rr does not take a
     problem with provisioner limits: rr_status() says it was never launched), and a handful of the seeded family's;
  b) the tamper matrix and the pinned one-sidedness through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  c) a batch of six what-ifs of a 24-node snapshot whose provisioner carries a limit, derived on the device against flattened one by one;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_limits.py runs the same kernels' source on the emulator."""
import numpy as np
import pytest

import audit_harness as H
import audit_limits_cases as LC
from karpenter_core_amd import scheduler as S

pytestmark = pytest.mark.gpu

GENUINE = {"capped before second": LC.capped_problem, "capped alone, two unscheduled": lambda: LC.capped_problem(pods=5, second=False), "one-sided": LC.one_sided_problem,
           "a limited template between two": LC.between_problem, "twelve names": LC.wide_names_problem, "negative from the start": LC.negative_problem}
GENUINE.update({"family %d" % seed: (lambda seed=seed: LC.family_problem(seed)) for seed in LC.FAMILY_SEEDS[:8]})


@pytest.mark.parametrize("name", list(GENUINE))
def test_genuine_results_are_clean(name):
    f = S.FlatProblem(GENUINE[name]())      # no flag asks for ks_pack: a provisioner with limits is not ks_pack_rr's
    try:
        f.solve(decode=False)
        assert f.rr_status() == (False, 0) and f.pack_width() > 0, (f.rr_status(), f.pack_width())
        dev = LC.assert_clean(S, f)
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} M {f.dims['M']} {LC.summary(dev)} ms {dev['ms']}")
        res = f.result_arrays()
        assert len(dev["pod_flags"]) == f.dims["P"] and len(dev["node_flags"]) == f.dims["E"] + res["n_new"] and dev["n_new"] == res["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((res["pod_node"] >= 0).sum()) and dev["limited_templates"] >= 1
    finally:
        f.close()


@pytest.fixture(scope="module")
def matrix():
    return dict(LC.run_tamper_matrix(S))


@pytest.mark.parametrize("name", LC.TAMPER_REPORT_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


@pytest.fixture(scope="module")
def one_sided():
    return dict(LC.run_one_sided(S))


@pytest.mark.parametrize("name", LC.ONE_SIDED_NAMES)
def test_one_sidedness_is_pinned(one_sided, name):
    assert one_sided[name] is True, one_sided[name]


def test_a_batch_of_derived_whatifs_over_a_limited_snapshot():
    for d in LC.run_whatifs(S):
        print(d)


@pytest.fixture(scope="module")
def shapes():
    return dict(LC.run_shapes(S))


@pytest.mark.parametrize("name", LC.SHAPE_NAMES)
def test_the_kernels_other_paths(shapes, name):
    """T = 1, 64, 65 and 130 with EXTRA and MISSING decided by the type in the last bit; 1, 64, 65 and 257 nodes of one limited template, one pod each, the edits on the
    last node (the prefix sums cross lanes, waves and tiles); a limited template between two unlimited ones; 12 resource names with the binding one last; R0 negative
    from the start; no limited template at all; n_new = 0; P = 1; limits = {}."""
    assert shapes[name] is True, shapes[name]


def test_flags_are_the_same_every_run():
    def edit(f):
        r, s = LC._claimable(f.result_arrays()), np.array(f.pod_seq(), dtype=np.int32)
        r["node_tmpl"][1] = 1
        LC._set_types(r, 0, 0x30)
        return r, s
    first = H.same_flags_every_run(LC.D, S, LC.capped_problem(), edit)
    assert first["n_pods_flagged"] >= 1
    first = H.same_flags_every_run(LC.D, S, LC.chain_problem(257))      # open[] by atomicMin, the counters by atomicAdd, 257 nodes through the scans
    assert first["exact_nodes"] == 257


def test_refusals():
    H.refusals(LC.D, S, LC.capped_problem(), totals=lambda out, f: (out.n_nodes, out.limited_templates, out.exact_nodes) == (3, 1, 2))
