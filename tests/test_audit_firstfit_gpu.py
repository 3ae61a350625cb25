"""(GPU) The audit's fourth pass on the device (include/ksolve.h ks_audit_firstfit_dev, KS_AUDIT_POD_FIT_*; kernels in karpenter_core_amd/csrc/ks_audit_firstfit.inc)
against its literal reference (tests/audit_firstfit_ref.py):
  a) genuine results are clean and not vacuously so -- every flag zero, bit for bit what the reference says, `checked`, `admitting_pairs` and `skipped_pods` included --
     over the problem list of tests/test_audit_spread_gpu.py with a few generic pods added, through ks_pack_rr and through ks_pack;
  b) a batch of what-ifs derived on the device against the same what-ifs flattened one by one;
  c) the tamper matrix through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_firstfit.py runs the same kernels' source on the emulator."""
import ctypes

import numpy as np
import pytest

import audit_firstfit_cases as FC
import audit_firstfit_ref as FR
import test_audit_spread_gpu as SG
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu

GENUINE = {name: (lambda make=make: FC.with_generic_pods(make())) for name, make in SG.GENUINE.items()}
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
    """tests/test_audit_spread_gpu.py's decorated snapshot: the what-ifs flattened one by one are clean by the reference and by the device; the device pass over the
    batch derived on the device -- the snapshot's classes, the removed nodes skipped -- finds the same, nothing, over as many pods and pairs, as many of them admitting."""
    import test_whatif_derived as WD
    its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
    sets = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]
    parsed = S.ParsedProblem(snap)
    flats = S.open_whatifs(parsed, pod_node, sets, derive=False)
    S.solve_batch(flats, decode=False)
    plain = [FC.assert_clean(S, f) for f in flats]
    batch = S.audit_firstfit_batch(flats)      # the batch form over flattened problems says what one call each said
    for b, p in zip(batch, plain):
        assert np.array_equal(b["pod_flags"], p["pod_flags"]) and FC.summary(b) == FC.summary(p)
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True)
    S.solve_batch_resident(derived)
    got = S.audit_firstfit_batch(derived)
    assert len(got) == len(sets)
    for d, p in zip(got, plain):
        print(FC.summary(d), FC.summary(p))
        assert not d["pod_flags"].any() and d["n_pods_flagged"] == 0
        assert len(d["pod_flags"]) == len(p["pod_flags"]) and FC.summary(d) == FC.summary(p)
    assert sum(d["checked"]["PODS"] for d in got) > 0
    with pytest.raises(S.KSolveError) as e:      # a claimed result on a derived view
        derived[0].audit_firstfit(claimed=flats[0].result_arrays(), pod_seq=np.zeros(len(plain[0]["pod_flags"]), dtype=np.int32))
    assert e.value.code == S.KS_ERR_UNSUPPORTED
    for f in flats + derived:
        f.close()


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


def test_flags_are_the_same_every_run():
    f = S.FlatProblem(FC.tamper_problem())
    f.solve(decode=False)
    name, claimed, seq, pod, bits, alone = FC.tampers(f.result_arrays(), f.pod_seq(), FR.problem_arrays(S, f))[1]
    runs = [f.audit_firstfit(claimed, seq) for _ in range(3)]
    assert all(np.array_equal(r["pod_flags"], runs[0]["pod_flags"]) and FC.summary(r) == FC.summary(runs[0]) for r in runs) and runs[0]["n_pods_flagged"] >= 1
    g = S.FlatProblem(W.config3(pods=700, sizes=10, seed=7))      # new nodes and many classes: open[] and first_*[] by atomicMin, the sums by atomicAdd
    g.solve(decode=False)
    runs = [g.audit_firstfit() for _ in range(3)]
    assert all(np.array_equal(r["pod_flags"], runs[0]["pod_flags"]) and FC.summary(r) == FC.summary(runs[0]) for r in runs) and runs[0]["checked"]["PODS"] > 0
    f.close(); g.close()


def test_refusals():
    ks, kh = S.libs()
    f = S.FlatProblem(FC.tamper_problem())
    f.upload(0)
    with pytest.raises(S.KSolveError) as e:      # nothing solved
        f.audit_firstfit()
    assert e.value.code == S.KS_ERR_INVALID
    f.solve(decode=False)
    kh.ksh_audit_firstfit.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(S._AuditFirstFitOut), ctypes.POINTER(ctypes.c_double)]
    hs = (ctypes.c_void_p * 1)(f._h)
    out = (S._AuditFirstFitOut * 1)()
    out[0].cap_pods, out[0].pod_flags = 64, None      # a table promised and not given
    assert kh.ksh_audit_firstfit(hs, 1, out, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_firstfit(hs, 1, None, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_firstfit(None, 1, out, None) == S.KS_ERR_INVALID
    out[0].cap_pods = 0      # the totals alone: no table needed
    assert kh.ksh_audit_firstfit(hs, 1, out, None) == S.KS_OK and out[0].n_pods == f.dims["P"] and out[0].truncated == S.KSH_AUDIT_TRUNCATED_PODS and out[0].checked[0] == f.dims["P"]
    ks.ks_audit_firstfit_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert ks.ks_audit_firstfit_dev(None, None, None) == S.KS_ERR_INVALID
    ks.ks_audit_firstfit_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert ks.ks_audit_firstfit_batch_dev(None, 1, None) == S.KS_ERR_INVALID
    res, seq = f.result_arrays(), f.pod_seq()
    many = dict(res, n_new=f.dims["P"] + 1)      # more new nodes than max_new_nodes
    with pytest.raises(S.KSolveError) as e:
        f.audit_firstfit(claimed=many, pod_seq=seq)
    assert e.value.code == S.KS_ERR_INVALID
    with pytest.raises(S.KSolveError) as e:      # no commit numbers
        f.audit_firstfit(claimed=res)
    assert e.value.code == S.KS_ERR_INVALID
    kh.ksh_audit_firstfit_claimed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(S._AuditFirstFitOut), ctypes.POINTER(ctypes.c_double)]
    assert kh.ksh_audit_firstfit_claimed(f._h, None, seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    ra = S._ResultArrays()      # the right dimensions and no arrays
    ra.n_pods, ra.n_existing, ra.types_words, ra.n_resources, ra.n_keys = f.dims["P"], f.dims["E"], (f.dims["T"] + 63) // 64, f.dims["R"], f.dims["K"]
    assert kh.ksh_audit_firstfit_claimed(f._h, ctypes.byref(ra), seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    f.close()
