"""The static feasibility grid (karpenter_core_amd/csrc/ksolve.hip: ks_grid_mc, ks_grid_types / ks_grid_types_wide), cell by cell.

grid[m][c] is filterInstanceTypesByRequirements (node.go:137-159) for a fresh node of template m that receives one pod of class c.  The reference is the CPU oracle, not the
product: for template m and a pod, `oracle.solve` of the one-provisioner, one-pod problem over the same catalogue, `extra_well_known` and daemonset pods; its
`new_nodes[0].instance_types` is the cell, no new node is an empty row.  (The grid knows nothing of provisioner limits: the reference problem carries none.)  Pods map to class
rows through `FlatProblem.pod_classes()` (kshost.h ksh_debug_pod_classes), never through request order.  Every comparison is bit-exact.

Three families: one problem per case through ks_feasibility_grid (`test_solo_grid_*`), row ranges (`test_row_ranges_*`), and the grid a BATCHED build leaves in every member
(`FlatProblem.built_grid()`, ksolve.h ks_debug_grid) against that member's own solo grid -- batches that mix grid widths TW, M * C, C and R, at the three wave targets
ks_solve_batch_dev uses (8192 for a batch of 2, 128 for 128, 64 for 256 and more).
"""
import dataclasses

import numpy as np
import pytest

from karpenter_core_amd import fake, scheduler as S, workloads as W
from karpenter_core_amd.model import (Container, Expr, Offering, Pod, Problem, Taint, Toleration, LABEL_ARCH, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME,
                                      LABEL_INSTANCE_TYPE, LABEL_OS, LABEL_ZONE, NO_SCHEDULE, REASON_NO_INSTANCE_TYPE, REASON_REQUIREMENTS, REASON_TAINTS,
                                      parse_quantity_milli)
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

Z = W.ZONES
TAINT_A, TAINT_B = Taint("grid-a", "true", NO_SCHEDULE), Taint("grid-b", "true", NO_SCHEDULE)
TOL_A = Toleration(key="grid-a", operator="Exists", effect=NO_SCHEDULE)
TOL_B = Toleration(key="grid-b", operator="Equal", value="true", effect=NO_SCHEDULE)
TOL_ALL = Toleration(operator="Exists")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def templates_in_grid_order(pr):
    """OrderByWeight (provisioner.go:132-136); the cases give every provisioner its own weight, so the order is total."""
    assert len({p.weight for p in pr.provisioners}) == len(pr.provisioners)
    return sorted(pr.provisioners, key=lambda p: -p.weight)


def reference_grid(pr, cls, C):
    """(uint64 [M, C, TW], int [M, C] why a row is empty -- REASON_* or 0) from the oracle: one solve per (template, pod).  Every pod of a class must give the class's row."""
    its = pr.instance_types
    idx = {it.name: t for t, it in enumerate(its)}
    tmpls = templates_in_grid_order(pr)
    tw = (len(its) + 63) // 64
    ref = np.zeros((len(tmpls), C, tw), dtype=np.uint64)
    why = np.zeros((len(tmpls), C), dtype=np.int64)
    seen = np.zeros((len(tmpls), C), dtype=bool)
    for m, prov in enumerate(tmpls):
        for i, pod in enumerate(pr.pods):
            c = int(cls[i])
            single = Problem(instance_types=its, provisioners=[dataclasses.replace(prov, limits=None)], pods=[pod], daemonset_pods=pr.daemonset_pods,
                             extra_well_known=pr.extra_well_known)
            want = O.solve(single)
            row = np.zeros(tw, dtype=np.uint64)
            reason = 0
            if want.new_nodes:
                assert len(want.new_nodes) == 1 and want.new_nodes[0].instance_types
                for name in want.new_nodes[0].instance_types:
                    row[idx[name] // 64] |= np.uint64(1 << (idx[name] % 64))
            else:
                assert want.unscheduled == [0]
                reason = want.reasons[0] & 0xF
            if seen[m, c]:
                assert (ref[m, c] == row).all() and why[m, c] == reason, f"pods of class {c} disagree in the reference (template {prov.name}, pod {pod.uid})"
            ref[m, c], why[m, c], seen[m, c] = row, reason, True
    assert seen.all(), "a class no pod of the problem maps to: a cell would go unchecked"
    return ref, why


def assert_same_grid(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        m, c, w = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError(f"{what}: {int((got != want).sum())} grid words differ; first at template {m}, class {c}, word {w}: got {int(got[m, c, w]):#018x}, want {int(want[m, c, w]):#018x}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
# catalogues, templates, pods
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def diagonal_type(name, cpu="4"):
    """Offers (spot, zone 2) and (on-demand, zone 1) only: a node held to zone 1 AND spot passes both of the type's requirements and still finds no offering (node.go:151)."""
    res = {"cpu": cpu, "memory": "16Gi", "pods": "40"}
    p = fake.price_from_resources(res)
    return fake.new_instance_type(name, res, [Offering("spot", Z[1], p), Offering("on-demand", Z[0], p), Offering("spot", Z[0], p, available=False)])


def ladder(sizes):
    """32 types per size: arch x os x four zone sets x two capacity-type sets."""
    return W._taint_catalogue(sizes, [[Z[0]], [Z[1]], [Z[2]], Z[:2]], [["spot", "on-demand"], ["on-demand"]])


def catalogue(T):
    if T in (1, 63, 190):
        return fake.instance_types(T)
    if T in (64, 128):
        return ladder(T // 32)
    if T == 65:
        return ladder(2) + [diagonal_type("diag-0")]
    if T == 129:
        return fake.instance_types(64) + ladder(2) + [diagonal_type("diag-0", "6")]
    if T == 257:
        return ladder(8) + [diagonal_type("diag-0")]
    raise ValueError(T)


def provisioners(its, M):
    """2..5 templates, heaviest first: taints, In / NotIn / Exists / DoesNotExist / Gt / Lt requirements, a custom label, an instance-type-name list and a type subset."""
    n = len(its)
    names = [it.name for it in its]
    all_ = [
        fake.provisioner("spot-a", n, weight=50, taints=[TAINT_A], requirements=[Expr(LABEL_CAPACITY_TYPE, "In", ["spot"])], labels={"team": "a"}),
        fake.provisioner("default", n, weight=40, requirements=[Expr(fake.LABEL_INTEGER, "Gt", ["1"]), Expr(fake.LABEL_INTEGER, "Lt", ["150"])]),
        fake.provisioner("ab-odd", weight=30, taints=[TAINT_A, TAINT_B], requirements=[Expr(LABEL_ZONE, "NotIn", [Z[0]]), Expr(fake.LABEL_EXOTIC, "DoesNotExist", [])],
                         instance_types=range(0, n, 2) if n > 1 else [0]),
        fake.provisioner("named", n, weight=20, requirements=[Expr(LABEL_INSTANCE_TYPE, "In", names[::3] + ["no-such-type"]), Expr(fake.LABEL_INSTANCE_SIZE, "Exists", [])]),
        fake.provisioner("plain", n, weight=10, requirements=[Expr(LABEL_INSTANCE_TYPE, "NotIn", names[1::4]), Expr(LABEL_OS, "In", ["linux", "windows"])], labels={"team": "b"}),
    ]
    return all_[:M]


def alloc_milli(it, res):
    return parse_quantity_milli(it.capacity[res]) - parse_quantity_milli(it.overhead.get(res, "0"))


def pod_menu(its, edge_type, n_extra=0):
    """At most 60 pods, one class each: what a pod can ask of a fresh node, one thing at a time and in a few combinations."""
    names = [it.name for it in its]
    pods = []

    def add(requests=None, **kw):
        pods.append(Pod(uid=f"g{len(pods):03d}", containers=[Container(requests=dict(requests or {"cpu": "100m", "memory": "64Mi"}))], **kw))
    add()
    add(tolerations=[TOL_A])
    add(tolerations=[TOL_A, TOL_B])
    add(tolerations=[TOL_ALL])
    add(tolerations=[TOL_B], node_selector={LABEL_ARCH: "amd64"})
    for k, v in ((LABEL_ARCH, "arm64"), (LABEL_OS, "windows"), (LABEL_ZONE, Z[2]), (LABEL_ZONE, Z[0]), (LABEL_CAPACITY_TYPE, "spot"), ("team", "a"), ("team", "c")):
        add(node_selector={k: v}, tolerations=[TOL_A])
    add(node_selector={LABEL_ZONE: Z[0], LABEL_CAPACITY_TYPE: "spot"}, tolerations=[TOL_ALL])      # the diagonal type: both requirements pass, no offering
    add(node_selector={LABEL_ZONE: Z[1], LABEL_CAPACITY_TYPE: "on-demand"})
    add(node_selector={LABEL_HOSTNAME: "some-node"}, tolerations=[TOL_ALL])                              # a concrete hostname: no fresh node (node.go:46)
    add(required_affinity=[[Expr(LABEL_HOSTNAME, "In", ["node-1", "node-2"])]])
    ra = [
        [Expr(LABEL_ZONE, "In", [Z[1], Z[2]])], [Expr(LABEL_ZONE, "NotIn", [Z[1]])], [Expr(LABEL_ZONE, "NotIn", Z[:3])], [Expr(LABEL_CAPACITY_TYPE, "NotIn", ["on-demand"])],
        [Expr(fake.LABEL_EXOTIC, "Exists", [])], [Expr(fake.LABEL_EXOTIC, "DoesNotExist", [])], [Expr(fake.LABEL_INSTANCE_SIZE, "In", ["large"])],
        [Expr(fake.LABEL_INSTANCE_SIZE, "NotIn", ["large"])], [Expr("team", "Exists", [])], [Expr("team", "DoesNotExist", [])], [Expr("team", "NotIn", ["a"])],
        [Expr(fake.LABEL_INTEGER, "Gt", ["8"])], [Expr(fake.LABEL_INTEGER, "Lt", ["8"])], [Expr(fake.LABEL_INTEGER, "Gt", ["2"]), Expr(fake.LABEL_INTEGER, "Lt", ["5"])],
        [Expr(fake.LABEL_INTEGER, "Gt", ["100"])], [Expr(fake.LABEL_INTEGER, "Lt", ["1"])], [Expr(fake.LABEL_INTEGER, "In", ["4", "6", "64"])],
        [Expr(fake.LABEL_INTEGER, "NotIn", ["4"]), Expr(LABEL_OS, "In", ["linux"])],
        [Expr(LABEL_INSTANCE_TYPE, "In", [names[0], names[-1], names[len(names) // 2]])], [Expr(LABEL_INSTANCE_TYPE, "NotIn", names[::2])],
        [Expr(LABEL_INSTANCE_TYPE, "In", names[-3:]), Expr(LABEL_CAPACITY_TYPE, "In", ["spot"])], [Expr(LABEL_INSTANCE_TYPE, "In", ["no-such-type"])],
        [Expr(LABEL_INSTANCE_TYPE, "Exists", [])],
    ]
    for i, term in enumerate(ra):
        add(required_affinity=[term], tolerations=[TOL_A] if i % 2 else [TOL_ALL])
    add(node_selector={LABEL_INSTANCE_TYPE: names[-1]}, tolerations=[TOL_ALL])
    add(node_selector={LABEL_INSTANCE_TYPE: names[0]})
    # fits: exactly Allocatable() of `edge_type` on cpu / on memory, and one milli-unit above (resources.go:138-145; the templates without daemon overhead show the edge itself)
    et = its[edge_type]
    cpu, mem = alloc_milli(et, "cpu"), alloc_milli(et, "memory")
    add({"cpu": f"{cpu}m", "memory": "64Mi"}, tolerations=[TOL_ALL])
    add({"cpu": f"{cpu + 1}m", "memory": "64Mi"}, tolerations=[TOL_ALL])
    add({"cpu": "100m", "memory": f"{mem}m"}, tolerations=[TOL_ALL])
    add({"cpu": "100m", "memory": f"{mem + 1}m"}, tolerations=[TOL_ALL])
    add({"cpu": f"{cpu}m", "memory": f"{mem}m", "pods": "1"}, tolerations=[TOL_A])
    add({"cpu": "100000", "memory": "64Mi"}, tolerations=[TOL_ALL])                                     # fits nothing
    add({"cpu": "100m", "memory": "64Mi", "example.com/unknown": "1"}, tolerations=[TOL_ALL])          # a resource no type has
    for i in range(n_extra):
        add({"cpu": f"{150 + i}m", "memory": "64Mi"})
    assert len(pods) <= 60
    return pods


WIDE_CORE = ("cpu", "memory", "pods")      # every other name of the wide catalogue can be 0 on a type


def daemonsets():
    """One daemonset that tolerates taint A only: the templates' daemon overhead differs (scheduler.go:250-267)."""
    return [Pod(uid="ds-0", tolerations=[TOL_A], containers=[Container(requests={"cpu": "500m", "memory": "100Mi"})])]


SOLO_CASES = {      # id -> (T, M, daemonsets, the type the exact-fit pods aim at)
    "T1": (1, 2, False, 0), "T63": (63, 3, True, 40), "T64": (64, 4, False, 33), "T65": (65, 5, True, 64), "T128": (128, 2, True, 100), "T129": (129, 5, False, 70),
    "T190": (190, 3, False, 150), "T257": (257, 4, True, 256),
}


def solo_problem(case):
    T, M, ds, edge = SOLO_CASES[case]
    its = catalogue(T)
    return Problem(instance_types=its, provisioners=provisioners(its, M), pods=pod_menu(its, edge, n_extra=10 if case == "T129" else 0), daemonset_pods=daemonsets() if ds else [],
                   extra_well_known=fake.EXTRA_WELL_KNOWN)


def wide_problem(names):
    """R = 9..12 resource names (ks_grid_types_wide).  Every extended name is requested by some pod, and for every extended name X one added type has plenty of
    everything but X: whichever resource indices the flattening gives the names, the types that lack a resource of index >= 8 fail `fits` only there."""
    base = W.wide_catalogue(names=names, pods=8, types=70 if names % 2 else 24, seed=names)
    its = list(base.instance_types)
    big = {n: "64" for n in W.WIDE_NAMES[:names]}
    big.update({"cpu": "96", "memory": "768Gi", "ephemeral-storage": "500Gi", "pods": "234"})
    extended = [n for n in W.WIDE_NAMES[:names] if n not in WIDE_CORE]
    its.append(fake.new_instance_type("full-house", resources=dict(big), architecture="amd64", operating_systems=["linux"]))
    its += [fake.new_instance_type(f"lacks-{k}", resources={**big, x: "0"}, architecture="amd64", operating_systems=["linux"]) for k, x in enumerate(extended)]
    n = len(its)
    provs = [fake.provisioner("gpu", weight=10, taints=[W.GPU_TAINT], instance_types=range(0, n, 3)), fake.provisioner("default", n, weight=5),
             fake.provisioner("ondemand", n, weight=1, requirements=[Expr(LABEL_CAPACITY_TYPE, "In", ["on-demand"])])]
    tol = [Toleration(key=W.GPU_TAINT.key, operator="Exists")]
    pods = []

    def add(requests, **kw):
        pods.append(Pod(uid=f"w{len(pods):03d}", containers=[Container(requests=requests)], **kw))
    add({"cpu": "100m"})
    add({"cpu": "100m"}, tolerations=tol)
    add({"cpu": "100m"}, tolerations=tol, node_selector={"team": "a"})      # a label no template defines: incompatible requirements
    add({"cpu": "100m"}, tolerations=tol, node_selector={LABEL_CAPACITY_TYPE: "spot"})
    for x in extended:
        add({"cpu": "1", x: "1"}, tolerations=tol)
        add({"cpu": "1", x: "3"})
    add({"cpu": "1", **{x: "1" for x in extended[-2:]}}, tolerations=tol)
    add({"cpu": "1", extended[-1]: "64"}, tolerations=tol)                # exactly `full-house`'s Allocatable(), and one milli-unit above
    add({"cpu": "1", extended[-1]: "64001m"}, tolerations=tol)
    add({"cpu": "2", "memory": "1Gi", "ephemeral-storage": "499Gi"}, tolerations=tol)
    add({"cpu": "2", "memory": "1Gi", "ephemeral-storage": "501Gi"}, tolerations=tol)
    assert len(pods) <= 60
    return Problem(instance_types=its, provisioners=provs, pods=pods, daemonset_pods=base.daemonset_pods, extra_well_known=fake.EXTRA_WELL_KNOWN)


_solo_cache = {}


def solo_case(case):
    """(problem, solo grid through ks_feasibility_grid, reference grid, reasons): computed once per case, shared, never changed."""
    if case not in _solo_cache:
        pr = wide_problem(int(case[1:])) if case.startswith("R") else solo_problem(case)
        fp = S.FlatProblem(pr)
        try:
            got, _ = fp.grid()
            cls = fp.pod_classes()
            ref, why = reference_grid(pr, cls, fp.dims["C"])
            dims = dict(fp.dims)
        finally:
            fp.close()
        for a in (got, ref, why):
            a.setflags(write=False)
        _solo_cache[case] = (pr, got, ref, why, dims)
    return _solo_cache[case]


def full_words(T):
    tw = (T + 63) // 64
    return np.array([(1 << min(64, T - 64 * w)) - 1 for w in range(tw)], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
# one problem per case: ks_feasibility_grid against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
NARROW = sorted(SOLO_CASES, key=lambda k: SOLO_CASES[k][0])
WIDE = ["R9", "R10", "R11", "R12"]


@pytest.mark.parametrize("case", NARROW + WIDE)
def test_solo_grid_equals_the_oracle_cell_by_cell(case):
    pr, got, ref, why, dims = solo_case(case)
    assert got.shape == (len(pr.provisioners), dims["C"], (len(pr.instance_types) + 63) // 64)
    if case.startswith("R"):
        assert dims["R"] == int(case[1:]) > 8
    else:
        assert dims["R"] <= 8 and dims["T"] == SOLO_CASES[case][0] and 2 <= dims["M"] <= 5
    assert_same_grid(got, ref, case)


@pytest.mark.parametrize("family", [NARROW, WIDE], ids=["narrow", "wide"])
def test_solo_references_are_not_vacuous(family):
    """What keeps the family above from passing on empty or trivial rows."""
    rows = nontrivial = 0
    reasons = set()
    words = {}
    for case in family:
        pr, _, ref, why, _ = solo_case(case)
        full = full_words(len(pr.instance_types))
        empty = ~ref.any(axis=2)
        rows += empty.size
        nontrivial += int((~empty & ~(ref == full).all(axis=2)).sum())
        reasons |= {int(x) for x in why[empty]}
        assert not why[~empty].any()
        for w in range(ref.shape[2]):
            words[(case, w)] = bool(ref[:, :, w].any())
    assert all(words.values()), f"grid words without a set bit in the reference: {[k for k, v in words.items() if not v]}"
    assert {REASON_TAINTS, REASON_REQUIREMENTS, REASON_NO_INSTANCE_TYPE} <= reasons
    assert nontrivial * 10 >= rows, (nontrivial, rows)


def test_solo_edges_land_where_they_were_aimed():
    """The cases contain what they were built for: the exact-fit pod keeps its type and the pod one milli-unit above loses it; the hostname class has no row; the diagonal
    type passes both requirements and has no offering; the type lacking a resource >= 8 fails only there."""
    pr, _, ref, why, _ = solo_case("T129")      # no daemonsets: the edge is the type's own Allocatable()
    fp = S.FlatProblem(pr)
    cls = fp.pod_classes()
    fp.close()
    by_uid = {p.uid: int(cls[i]) for i, p in enumerate(pr.pods)}
    edge = SOLO_CASES["T129"][3]
    bit = lambda m, uid, t: (int(ref[m, by_uid[uid], t // 64]) >> (t % 64)) & 1
    m = [p.name for p in templates_in_grid_order(pr)].index("plain")
    exact_cpu, over_cpu, exact_mem, over_mem = ("g%03d" % (len(pr.pods) - 17 + k) for k in range(4))
    assert pr.pods[len(pr.pods) - 17].containers[0].requests["cpu"] == f"{alloc_milli(pr.instance_types[edge], 'cpu')}m"
    assert bit(m, exact_cpu, edge) == 1 and bit(m, over_cpu, edge) == 0 and bit(m, exact_mem, edge) == 1 and bit(m, over_mem, edge) == 0
    hn = next(p.uid for p in pr.pods if p.node_selector.get(LABEL_HOSTNAME))
    assert not ref[:, by_uid[hn]].any() and (why[:, by_uid[hn]] != 0).all()
    diag = len(pr.instance_types) - 1
    held = next(p.uid for p in pr.pods if p.node_selector == {LABEL_ZONE: Z[0], LABEL_CAPACITY_TYPE: "spot"})
    free = next(p.uid for p in pr.pods if p.tolerations == [TOL_ALL] and not p.node_selector and not p.required_affinity and p.containers[0].requests == {"cpu": "100m", "memory": "64Mi"})
    assert bit(m, free, diag) == 1 and bit(m, held, diag) == 0
    for case in WIDE:
        prw, _, refw, _, _ = solo_case(case)
        fpw = S.FlatProblem(prw)
        clsw, res_names = fpw.pod_classes(), fpw.resource_names()
        fpw.close()
        tname = {it.name: t for t, it in enumerate(prw.instance_types)}
        extended = [n for n in W.WIDE_NAMES[:int(case[1:])] if n not in WIDE_CORE]
        mw = [p.name for p in templates_in_grid_order(prw)].index("default")
        wbit = lambda i, t: (int(refw[mw, int(clsw[i]), t // 64]) >> (t % 64)) & 1
        plain = next(i for i, p in enumerate(prw.pods) if p.containers[0].requests == {"cpu": "100m"} and p.tolerations)
        high = [x for x in res_names[8:] if x in extended]
        assert len(res_names) == int(case[1:]) and high, res_names
        for x in high:      # the type that lacks a resource of index >= 8: out for the pod that requests it, in for the pod that does not; the type that has it: in
            asks = next(i for i, p in enumerate(prw.pods) if p.containers[0].requests == {"cpu": "1", x: "1"})
            lacks = tname[f"lacks-{extended.index(x)}"]
            assert wbit(asks, tname["full-house"]) == 1 and wbit(asks, lacks) == 0 and wbit(plain, lacks) == 1, (case, x)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
# row ranges: ks_feasibility_grid_rows / _install
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def sentinel_rows(n, tw):
    """No grid word looks like these: every word differs, all have bits a T = 129 grid never sets in its last word."""
    return (np.arange(n * tw, dtype=np.uint64).reshape(n, tw) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(0xA5A5000000000000)


def test_row_ranges_compute_their_rows_and_leave_the_others_alone():
    pr, solo, _, _, dims = solo_case("T129")
    M, C, tw = solo.shape
    MC = M * C
    assert dims["T"] == 129 and MC >= 50
    want = solo.reshape(MC, tw)
    sent = sentinel_rows(MC, tw)
    assert not (sent == want).any()
    fp = S.FlatProblem(pr)
    try:
        fp.upload()
        with pytest.raises(S.KSolveError) as ei:      # nothing built yet: the read-only call refuses instead of building
            fp.built_grid()
        assert ei.value.code == S.KS_ERR_INVALID
        for lo, hi in ((0, 0), (0, 1), (7, 23), (MC - 1, MC)):
            fp.grid_install(0, MC, rows=sent)
            rows, _ = fp.grid_rows(lo, hi)
            assert rows.shape == (hi - lo, tw) and (rows == want[lo:hi]).all(), (lo, hi)
            with pytest.raises(S.KSolveError):          # a part of the rows is not a built grid
                fp.built_grid()
            fp.grid_install(0, 0, complete=True)
            now = fp.built_grid().reshape(MC, tw)
            assert (now[lo:hi] == want[lo:hi]).all(), (lo, hi)
            assert (now[:lo] == sent[:lo]).all() and (now[hi:] == sent[hi:]).all(), f"rows outside [{lo}, {hi}) changed"
        # the whole range in three uneven parts, installed into a fresh handle
        cuts = [0, 5, 31, MC]
        parts = [fp.grid_rows(a, b)[0] for a, b in zip(cuts, cuts[1:])]
    finally:
        fp.close()
    fresh = S.FlatProblem(pr)
    try:
        fresh.upload()
        fresh.grid_install(0, MC, rows=sent)
        for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
            fresh.grid_install(a, b, rows=parts[k], complete=k == 2)
        assert_same_grid(fresh.built_grid(), solo, "three installed parts")
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
# the grid a batched build leaves in every member, against the member's own solo grid
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def repro_problem(types, pods=50):
    """The issue's members: one default provisioner, pod i asks for 100 + i cores, so no two share a node and every class opens its own."""
    its = fake.instance_types(types)
    ps = [Pod(uid=f"big-{i:03d}", containers=[Container(requests={"cpu": str(100 + i), "memory": "64Mi"})]) for i in range(pods)]
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=ps, extra_well_known=fake.EXTRA_WELL_KNOWN)


def small_problem(types, pods, M=1, step=7):
    """`pods` classes with distinct small requests (they share nodes: the Solve stays short) over fake.instance_types(types), M templates."""
    its = fake.instance_types(types)
    ps = [Pod(uid=f"s-{i:04d}", containers=[Container(requests={"cpu": f"{100 + step * i}m", "memory": "64Mi"})],
              node_selector={LABEL_ZONE: Z[i % 3]} if i % 5 == 0 else {}) for i in range(pods)]
    provs = [fake.provisioner(f"p{m}", len(its), weight=10 * (M - m), requirements=[Expr(fake.LABEL_INTEGER, "Gt", [str(m)])] if m else []) for m in range(M)]
    return Problem(instance_types=its, provisioners=provs, pods=ps, extra_well_known=fake.EXTRA_WELL_KNOWN)


class TextOnce:
    """A problem many members of a batch are flattened from: its KSP1 text is written once (FlatProblem only asks for `to_ksp()`)."""

    def __init__(self, pr):
        self._text = pr.to_ksp()

    def to_ksp(self):
        return self._text


def solo_grid_of(pr):
    fp = S.FlatProblem(pr)
    try:
        return fp.grid()[0]
    finally:
        fp.close()


def assert_batch_grids_equal_solo(flats, solos, every_word=True):
    """Every member's grid as the batched build left it == that member's own solo grid (`solos[i]`, or built here on the member itself AFTER its batched grid was read).
    every_word: every grid word of every member has a set bit somewhere, so no word is compared as zeros against zeros."""
    widths = set()
    for i, f in enumerate(flats):
        got = f.built_grid()
        want = solos[i] if solos[i] is not None else f.grid()[0]
        assert_same_grid(got, want, f"member {i} (T {f.dims['T']}, M {f.dims['M']}, C {f.dims['C']}, R {f.dims['R']})")
        for w in range(want.shape[2] if every_word else 0):
            assert want[:, :, w].any(), f"member {i}: no set bit in grid word {w} of its solo grid"
        widths.add(want.shape[2])
    return widths


def close_all(flats):
    for f in flats:
        f.close()


_repro = {}


def repro_batch():
    """[B] + [A] * 127, solved once as a batch (decoded), A and B also solved alone, the grids read: shared by the grid test and the end-to-end test."""
    if not _repro:
        A, B = repro_problem(190), repro_problem(200)
        a_text = TextOnce(A)
        flats = [S.FlatProblem(B)] + [S.FlatProblem(a_text) for _ in range(127)]
        try:
            S.upload_batch(flats)
            res, _, _ = S.solve_batch(flats)
            grids = [f.built_grid() for f in flats]
        finally:
            close_all(flats)
        _repro.update(A=A, B=B, res=res, grids=grids, solo_grid={"A": solo_grid_of(A), "B": solo_grid_of(B)},
                      solo_res={"A": S.solve_problem(A), "B": S.solve_problem(B)})
    return _repro


def test_batch_of_128_repro_grids_equal_solo():
    """wave_target 128: the TW = 4 member alone would size the launch at 4 * 32 = 128 waves, the TW = 3 members need 3 * 43 = 129."""
    r = repro_batch()
    assert r["solo_grid"]["A"].shape == (1, 50, 3) and r["solo_grid"]["B"].shape == (1, 50, 4)
    assert r["solo_grid"]["A"][:, :, 1:].any(axis=(0, 1)).all()      # options 101..189 span words 1 and 2 (word 0: the other batches below)
    for i, g in enumerate(r["grids"]):
        assert_same_grid(g, r["solo_grid"]["B" if i == 0 else "A"], f"member {i}")


def test_batch_of_128_repro_solves_like_solo_and_the_oracle():
    r = repro_batch()
    want = {"A": O.solve(r["A"]), "B": O.solve(r["B"])}
    assert not want["A"].unscheduled and len(want["A"].new_nodes) == 50
    for k in "AB":
        assert r["solo_res"][k].canonical() == want[k].canonical() and r["solo_res"][k].reasons == want[k].reasons
    for i, got in enumerate(r["res"]):
        k = "B" if i == 0 else "A"
        assert got.canonical() == want[k].canonical(), f"member {i}: unscheduled {got.unscheduled}"
        assert got.reasons == want[k].reasons


def test_batch_of_128_control_of_equal_members():
    """128 x A: one width, so the launch bound was always right; the members equal the solo grid."""
    A = repro_problem(190)
    a_text = TextOnce(A)
    flats = [S.FlatProblem(a_text) for _ in range(128)]
    try:
        S.upload_batch(flats)
        S.solve_batch_resident(flats)
        solo = solo_grid_of(A)
        assert assert_batch_grids_equal_solo(flats, [solo] * 128, every_word=False) == {3}      # (pods of 100 cores and more: words 1 and 2 only)
    finally:
        close_all(flats)


def whatif_members(n):
    """n what-ifs flattened over one shared snapshot (ks_problem_upload_shared: the catalogue-derived tables are the snapshot's), T = 80."""
    its, prov, nodes, bound = W.cluster_snapshot(existing=12, sizes=2, seed=3)
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, with_cluster_pods=False)
    return S.open_whatifs(S.ParsedProblem(snap), pod_node, [[i, (i + 5) % 12] for i in range(n)], derive=False)


def mixed_members(n):
    """n members cycling over TW 1, 2, 3, 4, 5, 8, different M * C and C, one R > 8 problem beside R <= 8 ones, and what-ifs over a shared snapshot."""
    kinds = [small_problem(40, 9), small_problem(100, 30, M=2), small_problem(190, 23), small_problem(200, 16, M=3), small_problem(257, 45), small_problem(500, 12, M=2),
             small_problem(190, 15, M=3), wide_problem(10), small_problem(130, 64)]
    solo = [solo_grid_of(p) for p in kinds]
    texts = [TextOnce(p) for p in kinds]
    wi = whatif_members(3)
    flats, solos = list(wi), [None] * len(wi)
    for i in range(n - len(wi)):
        flats.append(S.FlatProblem(texts[i % len(kinds)]))
        solos.append(solo[i % len(kinds)])
    return flats, solos


@pytest.mark.parametrize("n", [2, 128, 256])
def test_mixed_width_batch_grids_equal_solo(n):
    """wave_target 8192 / 128 / 64.  At 64 a TW = 3 member with M * C >= 22 needs 66 waves beside a TW = 4 member's 64; at 128, TW = 3 and M * C >= 43 need 129."""
    if n == 2:
        flats, solos = [S.FlatProblem(small_problem(200, 16, M=3)), S.FlatProblem(wide_problem(9))], [None, None]
    else:
        flats, solos = mixed_members(n)
    try:
        assert len(flats) == n
        S.upload_batch(flats)
        S.solve_batch_resident(flats)
        widths = assert_batch_grids_equal_solo(flats, solos)
        assert widths == ({4, 2} if n == 2 else {1, 2, 3, 4, 5, 8})
        assert len({f.dims["C"] for f in flats}) > 1 and any(f.dims["R"] > 8 for f in flats) and any(f.dims["R"] <= 8 for f in flats)
    finally:
        close_all(flats)


def test_pair_at_wave_target_8192_grids_equal_solo():
    """A batch of 2 decodes with wave_target 8192: TW = 4 sizes the launch at 4 * 2048 = 8192 waves, a TW = 3 member with M * C >= 2731 needs 3 * 2731 = 8193.
    3 templates x 920 classes with distinct requests; only the grids are compared."""
    flats = [S.FlatProblem(small_problem(200, 920, M=3, step=1)), S.FlatProblem(small_problem(190, 920, M=3, step=1))]
    try:
        assert [f.dims["M"] * f.dims["C"] for f in flats] == [2760, 2760]
        S.upload_batch(flats)
        S.solve_batch_resident(flats)
        assert assert_batch_grids_equal_solo(flats, [None, None]) == {3, 4}
    finally:
        close_all(flats)
