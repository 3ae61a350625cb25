"""(GPU) The audit's third pass on the device (include/ksolve.h ks_audit_spread_dev, KS_AUDIT_POD_SPREAD; kernels in karpenter_core_amd/csrc/ks_audit_spread.inc)
against its literal reference (tests/audit_spread_ref.py):
  a) genuine results are clean and not vacuously so -- every flag zero, bit for bit what the reference says, `checked` and `exact_pairs` included -- over the
     topology-bearing problems of tests/test_audit_topology_gpu.py's list and the zonal spreads of tests/audit_spread_cases.py, through ks_pack_rr and through ks_pack;
  b) a batch of what-ifs derived on the device against the same what-ifs flattened one by one;
  c) the tamper matrix through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_spread.py runs the same kernels' source on the emulator."""
import ctypes

import numpy as np
import pytest

import audit_spread_cases as SC
import audit_spread_ref as SR
import audit_topo_cases as TC
import test_fuzz as F
import test_fuzz_mid as T
import test_problem_arrays as PA
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu

GENUINE = {
    "mid (topology, limits)": lambda: T.mid_problem(0),
    "node filter": lambda: PA.build_case("filter"),
    "existing nodes": lambda: PA.build_case("r3"),
    "fuzz 0": lambda: F.fuzz_problem(0), "fuzz 3": lambda: F.fuzz_problem(3), "fuzz 5": lambda: F.fuzz_problem(5), "fuzz 11": lambda: F.fuzz_problem(11), "fuzz 16": lambda: F.fuzz_problem(16),
    "config3": lambda: W.config3(pods=140, sizes=3, seed=1),
    "config3, 700 pods": lambda: W.config3(pods=700, sizes=10, seed=7),
    "a zonal spread on labelled nodes": lambda: SC.zonal(40, plain=3),
    "two keys": SC.two_keys,
}
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
    """tests/test_audit_topology_gpu.py's decorated snapshot: the what-ifs flattened one by one are clean by the reference and by the device; the device pass over the
    batch derived on the device finds the same -- nothing -- over as many placed pods and pairs, as many of them exact."""
    import test_whatif_derived as WD
    its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
    sets = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]
    parsed = S.ParsedProblem(snap)
    flats = S.open_whatifs(parsed, pod_node, sets, derive=False)
    S.solve_batch(flats, decode=False)
    plain = [SC.assert_clean(S, f) for f in flats]
    batch = S.audit_spread_batch(flats)      # the batch form over flattened problems says what one call each said
    for b, p in zip(batch, plain):
        assert np.array_equal(b["pod_flags"], p["pod_flags"]) and SC.summary(b) == SC.summary(p)
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True)
    S.solve_batch_resident(derived)
    got = S.audit_spread_batch(derived)
    assert len(got) == len(sets)
    for d, p in zip(got, plain):
        print(SC.summary(d), SC.summary(p))
        assert not d["pod_flags"].any() and d["n_pods_flagged"] == 0
        assert len(d["pod_flags"]) == len(p["pod_flags"]) and (d["n_new"], d["n_placed"], d["checked"], d["exact_pairs"]) == (p["n_new"], p["n_placed"], p["checked"], p["exact_pairs"])
    assert sum(d["checked"]["SPREAD"] for d in got) > 0
    assert SC.sliced_batch_says_the_same(S, derived, got)
    with pytest.raises(S.KSolveError) as e:      # a claimed result on a derived view
        derived[0].audit_spread(claimed=flats[0].result_arrays(), pod_seq=np.zeros(len(plain[0]["pod_flags"]), dtype=np.int32))
    assert e.value.code == S.KS_ERR_UNSUPPORTED
    for f in flats + derived:
        f.close()


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
    f = S.FlatProblem(SC.tamper_problem())
    f.solve(decode=False)
    name, claimed, seq, want = SC.tampers(f.result_arrays(), f.pod_seq())[1]
    runs = [f.audit_spread(claimed, seq) for _ in range(3)]
    assert all(np.array_equal(r["pod_flags"], runs[0]["pod_flags"]) and SC.summary(r) == SC.summary(runs[0]) for r in runs) and runs[0]["n_pods_flagged"] == 2
    g = S.FlatProblem(W.config3(pods=700, sizes=10, seed=7))      # new nodes: the pin table is built with atomicMin, the chunk table with atomicAdd
    g.solve(decode=False)
    runs = [g.audit_spread() for _ in range(3)]
    assert all(np.array_equal(r["pod_flags"], runs[0]["pod_flags"]) and SC.summary(r) == SC.summary(runs[0]) for r in runs) and runs[0]["checked"]["SPREAD"] > 0
    f.close(); g.close()


def test_refusals():
    ks, kh = S.libs()
    f = S.FlatProblem(SC.tamper_problem())
    f.upload(0)
    with pytest.raises(S.KSolveError) as e:      # nothing solved
        f.audit_spread()
    assert e.value.code == S.KS_ERR_INVALID
    f.solve(decode=False)
    kh.ksh_audit_spread.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(S._AuditSpreadOut), ctypes.POINTER(ctypes.c_double)]
    hs = (ctypes.c_void_p * 1)(f._h)
    out = (S._AuditSpreadOut * 1)()
    out[0].cap_pods, out[0].pod_flags = 64, None      # a table promised and not given
    assert kh.ksh_audit_spread(hs, 1, out, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_spread(hs, 1, None, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_spread(None, 1, out, None) == S.KS_ERR_INVALID
    out[0].cap_pods = 0      # the totals alone: no table needed
    assert kh.ksh_audit_spread(hs, 1, out, None) == S.KS_OK and out[0].n_pods == f.dims["P"] and out[0].truncated == S.KSH_AUDIT_TRUNCATED_PODS and out[0].checked[0] == f.dims["P"]
    ks.ks_audit_spread_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert ks.ks_audit_spread_dev(None, None, None) == S.KS_ERR_INVALID
    ks.ks_audit_spread_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert ks.ks_audit_spread_batch_dev(None, 1, None) == S.KS_ERR_INVALID
    res, seq = f.result_arrays(), f.pod_seq()
    many = dict(res, n_new=f.dims["P"] + 1)      # more new nodes than max_new_nodes
    with pytest.raises(S.KSolveError) as e:
        f.audit_spread(claimed=many, pod_seq=seq)
    assert e.value.code == S.KS_ERR_INVALID
    with pytest.raises(S.KSolveError) as e:      # no commit numbers
        f.audit_spread(claimed=res)
    assert e.value.code == S.KS_ERR_INVALID
    kh.ksh_audit_spread_claimed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(S._AuditSpreadOut), ctypes.POINTER(ctypes.c_double)]
    assert kh.ksh_audit_spread_claimed(f._h, None, seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    ra = S._ResultArrays()      # the right dimensions and no arrays
    ra.n_pods, ra.n_existing, ra.types_words, ra.n_resources, ra.n_keys = f.dims["P"], f.dims["E"], (f.dims["T"] + 63) // 64, f.dims["R"], f.dims["K"]
    assert kh.ksh_audit_spread_claimed(f._h, ctypes.byref(ra), seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    f.close()
