"""(GPU) The audit on the device (include/ksolve.h ks_audit_dev, KS_AUDIT_*; kernels in karpenter_core_amd/csrc/ks_audit.inc) against the literal reference audit
(tests/audit_ref.py):
  a) genuine results are clean -- every flag zero, and bit for bit what the reference audit says -- over the small generators through ks_pack_rr and through ks_pack,
     and at the sizes where the kernels take another path (a type word's edge and a second word, no existing node, no new node, one pod, a node whose pod list
     crosses the wave's stride and a block boundary, a batch of what-ifs derived on the device);
  b) the tamper matrix (tests/audit_cases.py) through the claimed form: one minimal edit per bit raises exactly that bit on exactly those indices;
  c) the refusals.
tests/test_audit.py runs the same kernels' source on the emulator."""
import numpy as np
import pytest

import audit_cases as C
import audit_harness as H
import audit_ref as A
import test_fuzz as F
import test_fuzz_mid as T
import test_problem_arrays as PA
from karpenter_core_amd import scheduler as S
from karpenter_core_amd import workloads as W
from karpenter_core_amd.model import Problem

pytestmark = pytest.mark.gpu


def _crowded():
    """One existing node holding 1 100 tiny pods: its pod list crosses the wave's stride (64) and every block boundary of the per-pod kernels (256)."""
    its = C.fake.instance_types(4)
    node = C._node("crowd", C.Z1, "8")
    node.available = {"cpu": "8", "memory": "64Gi", "pods": "2000"}
    return Problem(instance_types=its, provisioners=[C.fake.provisioner("open", len(its))], pods=[C._pod("tiny-%04d" % i, cpu="1m", mem="1Mi") for i in range(1100)],
                   nodes=[node], extra_well_known=C.fake.EXTRA_WELL_KNOWN)


def _all_on_existing():
    p = C.tamper_problem()
    return Problem(instance_types=p.instance_types, provisioners=p.provisioners, pods=p.pods[:7], nodes=p.nodes, extra_well_known=p.extra_well_known)


GENUINE = {
    "config3": lambda: W.config3(pods=140, sizes=3, seed=1),
    "config1": lambda: W.config1(pods=300, types=50, seed=42),
    "mid (topology, limits)": lambda: T.mid_problem(0),
    "hostname herd (topology)": lambda: W.hostname_herd(pods=200, labels=3, seed=3),
    "fuzz 0": lambda: F.fuzz_problem(0), "fuzz 3": lambda: F.fuzz_problem(3), "fuzz 5": lambda: F.fuzz_problem(5), "fuzz 11": lambda: F.fuzz_problem(11),
    "existing nodes": lambda: PA.build_case("r3"),
    "host ports": lambda: PA.build_case("ports"),
    "volume limits": lambda: PA.build_case("volumes"),
    "node filter": lambda: PA.build_case("filter"),
    "anti-affinity": lambda: PA.build_case("anti"),
    "instance-type and hostname selectors": lambda: PA.build_case("it_in"),
    "12 resource names": lambda: W.wide_catalogue(names=12, pods=60, types=24, existing=4, seed=2, dense=True),
    "T = 1": lambda: W.config1(pods=40, types=1, seed=1), "T = 64": lambda: W.config1(pods=80, types=64, seed=2),
    "T = 65": lambda: W.config1(pods=80, types=65, seed=3), "T = 130": lambda: W.config1(pods=80, types=130, seed=4),
    "P = 1": lambda: W.config1(pods=1, types=8, seed=5),
    "n_new = 0": _all_on_existing,
    "1 100 pods on one existing node": _crowded,
    "the tamper matrix's problem": C.tamper_problem,
}


@pytest.mark.parametrize("no_rr", [False, True], ids=["ks_pack_rr", "ks_pack"])
@pytest.mark.parametrize("name", list(GENUINE))
def test_genuine_results_are_clean(name, no_rr):
    f = S.FlatProblem(GENUINE[name](), flags=S.KS_FLAG_NO_RR if no_rr else 0)
    try:
        f.solve(decode=False)
        dev = C.assert_clean(S, f)
        res = f.result_arrays()
        print(f"{name}: P {f.dims['P']} E {f.dims['E']} T {f.dims['T']} R {f.dims['R']} n_new {dev['n_new']} unscheduled {dev['n_unscheduled']} rr {f.rr_status()} audit ms {dev['ms']}")
        assert dev["n_new"] == res["n_new"] and dev["n_unscheduled"] == len(res["unscheduled"])
        assert len(dev["pod_flags"]) == f.dims["P"] and len(dev["node_flags"]) == f.dims["E"] + res["n_new"]
        if name == "n_new = 0":
            assert res["n_new"] == 0 and f.dims["E"] > 0
        if name.startswith("T = ") or name == "P = 1":
            assert f.dims["E"] == 0 and f.dims["T"] == (8 if name == "P = 1" else int(name[4:])) and res["n_new"] > 0
        if name == "1 100 pods on one existing node":
            assert int((res["pod_node"] == 0).sum()) == 1100
        if name == "12 resource names":
            assert f.dims["R"] == 12
    finally:
        f.close()


def test_a_batch_of_derived_whatifs_is_clean():
    """What-ifs derived on the device have no flattening of their own to restate the audit over: the same what-ifs flattened one by one -- the same results, which
    tests/test_whatif_derived.py pins -- are clean by the reference audit and by the device, and the device audit of the derived batch, one launch sequence over
    the results where they lie, finds the same: nothing, over as many pods and nodes."""
    its, prov, nodes, bound = W.cluster_snapshot(existing=24, sizes=5, seed=11, spare_pod_slots=2)      # (full by pod count: most what-ifs need new nodes)
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
    sets = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]
    flats = S.open_whatifs(snap, pod_node, sets, derive=False)
    S.upload_batch(flats)
    S.solve_batch(flats, decode=False)
    plain = [C.assert_clean(S, f) for f in flats]
    derived = S.open_whatifs(S.ParsedProblem(snap), pod_node, sets, derive=True)
    S.solve_batch_resident(derived)
    got = S.audit_batch(derived)
    assert len(got) == len(sets)
    for d, p, cs in zip(got, plain, sets):
        assert not d["pod_flags"].any() and not d["node_flags"].any() and d["n_pods_flagged"] == 0 and d["n_nodes_flagged"] == 0
        assert len(d["pod_flags"]) == len(p["pod_flags"]) and d["n_new"] == p["n_new"] and d["n_unscheduled"] == p["n_unscheduled"]
        assert len(d["node_flags"]) == 24 + d["n_new"] and len(p["node_flags"]) == 24 - len(cs) + p["n_new"]      # (a derived what-if keeps the rows of the nodes that left)
    assert sum(1 for d in got if d["n_new"] > 0) >= 3, [d["n_new"] for d in got]
    batch = S.audit_batch(flats)      # the batch form over flattened problems says what one call each said
    for b, p in zip(batch, plain):
        assert np.array_equal(b["pod_flags"], p["pod_flags"]) and np.array_equal(b["node_flags"], p["node_flags"])
    with pytest.raises(S.KSolveError) as e:      # c) a claimed result on a derived view
        derived[0].audit(claimed=flats[0].result_arrays())
    assert e.value.code == S.KS_ERR_UNSUPPORTED
    for f in flats + derived:
        f.close()


@pytest.fixture(scope="module")
def matrix():
    return dict(C.run_tamper_matrix(S))


@pytest.mark.parametrize("name", C.TAMPER_NAMES)
def test_tamper_matrix(matrix, name):
    assert matrix[name] is True, matrix[name]


def test_the_matrix_is_the_list(matrix):
    assert list(matrix) == C.TAMPER_NAMES


def test_flags_are_the_same_every_run():
    first = H.same_flags_every_run(C.D, S, C.tamper_problem(), lambda f: (C.tampers(f.result_arrays(), A.problem_arrays(S, f))[4][1],))
    assert first["n_pods_flagged"] == 2


def test_refusals():
    H.refusals(C.D, S, C.tamper_problem())
