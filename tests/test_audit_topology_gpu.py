"""(GPU) The audit's second pass on the device (include/ksolve.h ks_audit_topology_dev, KS_AUDIT_POD_SEQ .. KS_AUDIT_POD_HOSTNAME_SPREAD; kernels in
karpenter_core_amd/csrc/ks_audit_topo.inc) against its literal reference (tests/audit_topo_ref.py):
  a) genuine results are clean and not vacuously so -- every flag zero, bit for bit what the reference says, `checked` included -- over the topology-bearing problems of
     tests/test_audit_gpu.py's list and the leaders-and-followers problem, through ks_pack_rr and through ks_pack; over the set every rule evaluated something;
  b) a batch of what-ifs derived on the device, with the snapshot's bound pods carrying terms, against the same what-ifs flattened one by one;
  c) the tamper matrix (tests/audit_topo_cases.py) through the claimed form, the commit numbers read from ksh_placement_rows and edited;
  d) the shapes where the kernels take another path; the same flags every run; the refusals.
tests/test_audit_topology.py runs the same kernels' source on the emulator."""
import numpy as np
import pytest

import audit_harness as H
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


def test_a_batch_of_derived_whatifs_is_clean():
    """tests/audit_harness.py's decorated snapshot: the device pass over the batch derived on the device -- the what-ifs' own group tables -- finds what the what-ifs
    flattened one by one say, nothing, over as many placed pods and what each rule evaluated (the groups are the snapshot's in a derived what-if: the skipped ones are not)."""
    H.derived_whatifs_are_clean(TC.D, S, same=lambda d: (d["n_new"], d["n_placed"], d["checked"]), examined=lambda d: sum(d["checked"][k] for k in TR.RULES[1:]))


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
    # the narrow-key rule: the table of least commit numbers is built with atomicMin
    first = H.same_flags_every_run(TC.D, S, TC.tamper_problem(), lambda f: TC.tampers(f.result_arrays(), f.pod_seq())[4][1:3])
    assert first["n_pods_flagged"] == 1
    H.same_flags_every_run(TC.D, S, T.mid_problem(0))


def test_refusals():
    H.refusals(TC.D, S, TC.tamper_problem())
