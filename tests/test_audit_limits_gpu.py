"""(GPU) The audit's fifth pass on the device (include/ksolve.h ks_audit_limits_dev, KS_AUDIT_NODE_LIMIT_*, KS_AUDIT_POD_LIMIT_TEMPLATE; kernels in
karpenter_core_amd/csrc/ks_audit_limits.inc) against its literal reference (tests/audit_limits_ref.py):
  a) the genuine problems are clean -- every flag zero, bit for bit what the reference says, every counter included -- through ks_pack (ks_pack_rr does not take a
     problem with provisioner limits: rr_status() says it was never launched), and a handful of the seeded family's;
  b) the tamper matrix and the pinned one-sidedness through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  c) a batch of six what-ifs of a 24-node snapshot whose provisioner carries a limit, derived on the device against flattened one by one;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_limits.py runs the same kernels' source on the emulator."""
import ctypes

import numpy as np
import pytest

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
    f = S.FlatProblem(LC.capped_problem())
    f.solve(decode=False)
    r, s = LC._claimable(f.result_arrays()), np.array(f.pod_seq(), dtype=np.int32)
    r["node_tmpl"][1] = 1
    LC._set_types(r, 0, 0x30)
    runs = [f.audit_limits(r, s) for _ in range(3)]
    assert all(np.array_equal(x["pod_flags"], runs[0]["pod_flags"]) and np.array_equal(x["node_flags"], runs[0]["node_flags"]) and LC.summary(x) == LC.summary(runs[0]) for x in runs)
    assert runs[0]["n_pods_flagged"] >= 1
    g = S.FlatProblem(LC.chain_problem(257))      # open[] by atomicMin, the counters by atomicAdd, 257 nodes through the scans
    g.solve(decode=False)
    runs = [g.audit_limits() for _ in range(3)]
    assert all(np.array_equal(x["pod_flags"], runs[0]["pod_flags"]) and np.array_equal(x["node_flags"], runs[0]["node_flags"]) and LC.summary(x) == LC.summary(runs[0]) for x in runs)
    assert runs[0]["exact_nodes"] == 257
    f.close(); g.close()


def test_refusals():
    ks, kh = S.libs()
    f = S.FlatProblem(LC.capped_problem())
    f.upload(0)
    with pytest.raises(S.KSolveError) as e:      # nothing solved
        f.audit_limits()
    assert e.value.code == S.KS_ERR_INVALID
    f.solve(decode=False)
    kh.ksh_audit_limits.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(S._AuditLimitsOut), ctypes.POINTER(ctypes.c_double)]
    hs = (ctypes.c_void_p * 1)(f._h)
    out = (S._AuditLimitsOut * 1)()
    out[0].cap_pods, out[0].pod_flags = 64, None      # a table promised and not given
    assert kh.ksh_audit_limits(hs, 1, out, None) == S.KS_ERR_INVALID
    out[0].cap_pods, out[0].cap_nodes, out[0].node_flags = 0, 64, None
    assert kh.ksh_audit_limits(hs, 1, out, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_limits(hs, 1, None, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_limits(None, 1, out, None) == S.KS_ERR_INVALID
    out[0].cap_nodes = 0      # the totals alone: no table needed
    assert kh.ksh_audit_limits(hs, 1, out, None) == S.KS_OK and out[0].n_pods == f.dims["P"] and out[0].n_nodes == 3 and out[0].checked[0] == f.dims["P"]
    assert out[0].truncated == S.KSH_AUDIT_TRUNCATED_PODS | S.KSH_AUDIT_TRUNCATED_NODES and out[0].limited_templates == 1 and out[0].exact_nodes == 2
    ks.ks_audit_limits_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert ks.ks_audit_limits_dev(None, None, None) == S.KS_ERR_INVALID
    ks.ks_audit_limits_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert ks.ks_audit_limits_batch_dev(None, 1, None) == S.KS_ERR_INVALID
    res, seq = f.result_arrays(), f.pod_seq()
    many = dict(res, n_new=f.dims["P"] + 1)      # more new nodes than max_new_nodes
    with pytest.raises(S.KSolveError) as e:
        f.audit_limits(claimed=many, pod_seq=seq)
    assert e.value.code == S.KS_ERR_INVALID
    with pytest.raises(S.KSolveError) as e:      # no commit numbers
        f.audit_limits(claimed=res)
    assert e.value.code == S.KS_ERR_INVALID
    kh.ksh_audit_limits_claimed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(S._AuditLimitsOut), ctypes.POINTER(ctypes.c_double)]
    assert kh.ksh_audit_limits_claimed(f._h, None, seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    ra = S._ResultArrays()      # the right dimensions and no arrays
    ra.n_pods, ra.n_existing, ra.types_words, ra.n_resources, ra.n_keys = f.dims["P"], f.dims["E"], (f.dims["T"] + 63) // 64, f.dims["R"], f.dims["K"]
    assert kh.ksh_audit_limits_claimed(f._h, ctypes.byref(ra), seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    f.close()
