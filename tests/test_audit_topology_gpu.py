"""(GPU) The audit's second pass on the device (include/ksolve.h ks_audit_topology_dev, KS_AUDIT_POD_SEQ .. KS_AUDIT_POD_HOSTNAME_SPREAD; kernels in
karpenter_core_amd/csrc/ks_audit_topo.inc) against its literal reference (tests/audit_topo_ref.py):
  a) genuine results are clean and not vacuously so -- every flag zero, bit for bit what the reference says, `checked` included -- over the topology-bearing problems of
     tests/test_audit_gpu.py's list and the leaders-and-followers problem, through ks_pack_rr and through ks_pack; over the set every rule evaluated something;
  b) a batch of what-ifs derived on the device, with the snapshot's bound pods carrying terms, against the same what-ifs flattened one by one;
  c) the tamper matrix (tests/audit_topo_cases.py) through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_topology.py runs the same kernels' source on the emulator."""
import ctypes

import numpy as np
import pytest

import audit_topo_cases as TC
import audit_topo_ref as TR
import test_fuzz as F
import test_fuzz_mid as T
import test_problem_arrays as PA
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W

pytestmark = pytest.mark.gpu

GENUINE = {
    "mid (topology, limits)": lambda: T.mid_problem(0),
    "hostname herd": lambda: W.hostname_herd(pods=200, labels=3, seed=3),
    "anti-affinity": lambda: PA.build_case("anti"),
    "node filter": lambda: PA.build_case("filter"),
    "existing nodes": lambda: PA.build_case("r3"),
    "fuzz 0": lambda: F.fuzz_problem(0), "fuzz 3": lambda: F.fuzz_problem(3), "fuzz 5": lambda: F.fuzz_problem(5), "fuzz 11": lambda: F.fuzz_problem(11),
    "config3": lambda: W.config3(pods=140, sizes=3, seed=1),
    "leaders and followers": TC.leaders_and_followers,
    "the tamper matrix's problem": TC.tamper_problem,
}
CHECKED = {}      # (name, kernel) -> checked[], filled by the test below and summed by the one after it


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name", list(GENUINE))
def test_genuine_results_are_clean(name, no_rr):
    f = S.FlatProblem(GENUINE[name](), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev = TC.assert_clean(S, f)
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} n_new {dev['n_new']} placed {dev['n_placed']} rr {f.rr_status()} checked {dev['checked']} skipped {dev['skipped_groups']} ms {dev['ms']}")
        assert len(dev["pod_flags"]) == f.dims["P"] and dev["n_new"] == f.result_arrays()["n_new"]
        assert dev["checked"]["SEQ"] == dev["n_placed"] == int((f.result_arrays()["pod_node"] >= 0).sum())
        CHECKED[(name, no_rr)] = dev["checked"]
    finally:
        f.close()


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
def test_the_clean_results_were_not_clean_vacuously(no_rr):
    """Over the set, every rule evaluated something."""
    got = [CHECKED[(n, no_rr)] for n in GENUINE if (n, no_rr) in CHECKED]
    assert len(got) == len(GENUINE), "runs after test_genuine_results_are_clean"
    total = {k: sum(c[k] for c in got) for k in TR.RULES}
    print(total)
    assert all(v > 0 for v in total.values()), total
    generators = {k: sum(CHECKED[(n, no_rr)][k] for n in GENUINE if n not in ("leaders and followers", "the tamper matrix's problem")) for k in TR.RULES}
    assert generators["ANTI_AFFINITY"] > 0 and generators["HOSTNAME_SPREAD"] > 0, generators


def derived_batch_is_clean(S):
    """tests/test_audit_gpu.py's snapshot shape, its bound pods carrying terms (tests/test_whatif_derived.py's decoration: spread, affinity, required anti-affinity
    over the hostname and the zone): the what-ifs flattened one by one are clean by the reference and by the device; the device pass over the batch derived on the
    device -- one launch sequence over the results where they lie, the what-ifs' own group tables -- finds the same: nothing, over as many placed pods."""
    import test_whatif_derived as WD
    its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
    sets = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]
    parsed = S.ParsedProblem(snap)
    flats = S.open_whatifs(parsed, pod_node, sets, derive=False)
    S.solve_batch(flats, decode=False)
    plain = [TC.assert_clean(S, f) for f in flats]
    batch = S.audit_topology_batch(flats)      # the batch form over flattened problems says what one call each said
    for b, p in zip(batch, plain):
        assert np.array_equal(b["pod_flags"], p["pod_flags"]) and b["checked"] == p["checked"] and b["skipped_groups"] == p["skipped_groups"]
    derived = S.open_whatifs(parsed, pod_node, sets, derive=True)
    S.solve_batch_resident(derived)
    got = S.audit_topology_batch(derived)
    assert len(got) == len(sets)
    for d, p in zip(got, plain):
        print(d["checked"], p["checked"], d["skipped_groups"], p["skipped_groups"])
        assert not d["pod_flags"].any() and d["n_pods_flagged"] == 0
        # comparable: the pods, where they went, what each rule evaluated (the groups are the snapshot's in a derived what-if: the skipped ones are not)
        assert len(d["pod_flags"]) == len(p["pod_flags"]) and d["n_new"] == p["n_new"] and d["n_placed"] == p["n_placed"] and d["checked"] == p["checked"]
    assert sum(sum(d["checked"][k] for k in TR.RULES[1:]) for d in got) > 0 and sum(sum(p["checked"][k] for k in TR.RULES[1:]) for p in plain) > 0
    with pytest.raises(S.KSolveError) as e:      # a claimed result on a derived view
        derived[0].audit_topology(claimed=flats[0].result_arrays(), pod_seq=np.zeros(len(plain[0]["pod_flags"]), dtype=np.int32))
    assert e.value.code == S.KS_ERR_UNSUPPORTED
    for f in flats + derived:
        f.close()


def test_a_batch_of_derived_whatifs_is_clean():
    derived_batch_is_clean(S)


@pytest.fixture(scope="module")
def matrix():
    return dict(TC.run_tamper_matrix(S))


@pytest.mark.parametrize("name", TC.TAMPER_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


@pytest.fixture(scope="module")
def shapes():
    return dict(TC.run_shape_tampers(S))


@pytest.mark.parametrize("name", TC.SHAPE_TAMPER_NAMES)
def test_violations_at_the_kernels_edges(shapes, name):
    """A topology key with 64 values and the violation in value id 63; a pod constrained by 24 groups and the violation in the last."""
    assert shapes[name] is True, shapes[name]


def test_a_node_whose_list_crosses_the_waves_stride_and_the_lds_tile():
    """1 100 tiny pods on one existing node under a self-selecting hostname spread with maxSkew 1 100: clean, 1 100 pairs evaluated.  The 1 101st, which the Solve gave a
    machine of its own, claimed onto the node: exactly the last of the 1 101 by commit number carries HOSTNAME_SPREAD."""
    f = S.FlatProblem(TC.crowded(1))
    f.solve(decode=False)
    dev = TC.assert_clean(S, f)
    res, seq = f.result_arrays(), f.pod_seq()
    on = res["pod_node"] == 0
    assert int(on.sum()) == 1100 and res["n_new"] == 1 and dev["checked"]["HOSTNAME_SPREAD"] == 1101
    extra = int(np.nonzero(~on)[0][0])
    res = {k: v for k, v in res.items() if k != "key_value"}
    res["pod_node"][extra] = 0
    dev, flags, _ = TC.compare(S, f, res, seq)
    last = int(np.argmax(seq))
    assert {int(i): int(flags[i]) for i in np.nonzero(flags)[0]} == {last: TR.BITS["HOSTNAME_SPREAD"]}
    assert dev["pod_bit_count"]["HOSTNAME_SPREAD"] == 1 and dev["n_pods_flagged"] == 1
    f.close()


@pytest.mark.parametrize("name,make,checked,n_new", [("P = 1", lambda: TC.plain(1), [1, 0, 0, 0], 1), ("G = 0 and n_new = 0", lambda: TC.plain(3, True), [3, 0, 0, 0], 0)])
def test_nothing_to_check(name, make, checked, n_new):
    f = S.FlatProblem(make())
    f.solve(decode=False)
    dev = TC.assert_clean(S, f)
    assert [dev["checked"][k] for k in TR.RULES] == checked and dev["n_new"] == n_new and dev["skipped_groups"] == 0
    f.close()


def test_flags_are_the_same_every_run():
    f = S.FlatProblem(TC.tamper_problem())
    f.solve(decode=False)
    name, claimed, seq, want = TC.tampers(f.result_arrays(), f.pod_seq())[4]      # the narrow-key rule: the table of least commit numbers is built with atomicMin
    runs = [f.audit_topology(claimed, seq) for _ in range(3)]
    assert all(np.array_equal(r["pod_flags"], runs[0]["pod_flags"]) and r["checked"] == runs[0]["checked"] for r in runs) and runs[0]["n_pods_flagged"] == 1
    g = S.FlatProblem(T.mid_problem(0))
    g.solve(decode=False)
    runs = [g.audit_topology() for _ in range(3)]
    assert all(np.array_equal(r["pod_flags"], runs[0]["pod_flags"]) and r["checked"] == runs[0]["checked"] for r in runs)
    f.close(); g.close()


def test_refusals():
    ks, kh = S.libs()
    f = S.FlatProblem(TC.tamper_problem())
    f.upload(0)
    with pytest.raises(S.KSolveError) as e:      # nothing solved
        f.audit_topology()
    assert e.value.code == S.KS_ERR_INVALID
    f.solve(decode=False)
    kh.ksh_audit_topology.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(S._AuditTopologyOut), ctypes.POINTER(ctypes.c_double)]
    hs = (ctypes.c_void_p * 1)(f._h)
    out = (S._AuditTopologyOut * 1)()
    out[0].cap_pods, out[0].pod_flags = 64, None      # a table promised and not given
    assert kh.ksh_audit_topology(hs, 1, out, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_topology(hs, 1, None, None) == S.KS_ERR_INVALID
    assert kh.ksh_audit_topology(None, 1, out, None) == S.KS_ERR_INVALID
    out[0].cap_pods = 0      # the totals alone: no table needed
    assert kh.ksh_audit_topology(hs, 1, out, None) == S.KS_OK and out[0].n_pods == f.dims["P"] and out[0].truncated == S.KSH_AUDIT_TRUNCATED_PODS and out[0].checked[0] == f.dims["P"]
    ks.ks_audit_topology_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert ks.ks_audit_topology_dev(None, None, None) == S.KS_ERR_INVALID
    ks.ks_audit_topology_batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert ks.ks_audit_topology_batch_dev(None, 1, None) == S.KS_ERR_INVALID
    res, seq = f.result_arrays(), f.pod_seq()
    many = dict(res, n_new=f.dims["P"] + 1)      # more new nodes than max_new_nodes
    with pytest.raises(S.KSolveError) as e:
        f.audit_topology(claimed=many, pod_seq=seq)
    assert e.value.code == S.KS_ERR_INVALID
    with pytest.raises(S.KSolveError) as e:      # no commit numbers
        f.audit_topology(claimed=res)
    assert e.value.code == S.KS_ERR_INVALID
    kh.ksh_audit_topology_claimed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(S._AuditTopologyOut), ctypes.POINTER(ctypes.c_double)]
    assert kh.ksh_audit_topology_claimed(f._h, None, seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    ra = S._ResultArrays()      # the right dimensions and no arrays
    ra.n_pods, ra.n_existing, ra.types_words, ra.n_resources, ra.n_keys = f.dims["P"], f.dims["E"], (f.dims["T"] + 63) // 64, f.dims["R"], f.dims["K"]
    assert kh.ksh_audit_topology_claimed(f._h, ctypes.byref(ra), seq.ctypes.data, out, None) == S.KS_ERR_INVALID
    f.close()
