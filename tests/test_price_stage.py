"""The consolidation price stage kernels of csrc/ksolve.hip against their literal restatements in oracle/consolidation_ref.py, on catalogues made to break them:
  ks_price_filter   filterByPrice over worstLaunchPrice (deprovisioning/helpers.go:148-157, 292-315)      vs CR.filter_by_price
  ks_launch_pick    the in-memory provider's cheapest-offering pick (fake/cloudprovider.go:72-84)         vs CR.launch_pick
  ks_types_subset   instanceTypesAreSubset (helpers.go:118-122)                                         vs CR.instance_types_are_subset
The catalogues repeat (zone, capacity type) pairs at different prices (the encoder keeps the maximum for worstLaunchPrice and the minimum for Cheapest), mark
offerings unavailable, draw prices from a small set with 0.0 and two doubles one ulp apart, and vary the capacity types (a third one, none called spot); pods carry
In / NotIn selectors on zone and capacity type, so every new node has requirements of its own.  Ceilings sit exactly on every worst price (the compare is a strict <)
and one ulp above it.  Index edges: 64 zone x capacity-type pairs (bit 63), T = 65, T > 4096 (a lane walks several words), one call over problems of different T.

Every case runs twice: unmarked, on the emulator build of the kernels (tests/sim) in a child process -- the pytest process keeps the real libraries --, and marked
`gpu`, on the device.  `device_run` is the part that needs the kernels; the comparison with the reference happens here, against the oracle's own Solve."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd import fake
from karpenter_core_amd.model import LABEL_CAPACITY_TYPE as CT, LABEL_ZONE as ZONE, Container, Expr, Offering, Pod, Problem
from oracle import consolidation_ref as CR
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# a small set, so that prices tie across types and within a type; 0.5 and the next double above it are merged by a float32 or fused path
PRICES = [0.0, 0.25, 0.5, 0.5000000000000001, 0.75, 1.0, 1.5, 3.0]


def price_catalogue(seed, types=40, zones=3, cts=("spot", "on-demand"), pods=40):
    """A seeded Solve problem for the price stage: 1-6 offerings per type (the last type: one in every pair), about a third of them repeating a (zone,
    capacity type) pair of the same type at another price, about 15 % unavailable; pods with zone / capacity-type selectors that name only the catalogue's own
    zones and capacity types (a capacity type a pod names joins the universe, and "no spot" must stay without one)."""
    rs = np.random.RandomState(seed)
    zs = [f"pz-{i:02d}" for i in range(zones)]
    its = []
    for t in range(types):
        offs = []
        if t < zones:          # every zone in the universe (32 zones x 2 capacity types fill the 64 pairs), and the last one often: its pairs are the high bits
            offs.append(Offering(cts[t % len(cts)], zs[t], PRICES[int(rs.randint(len(PRICES)))], True))
        elif t == types - 1:   # the last type offers every pair: an option of most nodes, on the far side of every word edge
            offs += [Offering(c, z, PRICES[int(rs.randint(len(PRICES)))], True) for z in zs for c in cts]
        elif t % 3 == 0:
            offs.append(Offering(cts[int(rs.randint(len(cts)))], zs[-1], PRICES[int(rs.randint(len(PRICES)))], True))
        for _ in range(int(rs.randint(1, 7)) - len(offs)):
            if offs and rs.rand() < 0.35:          # the same pair again, at another price
                o = offs[int(rs.randint(len(offs)))]
                price = PRICES[int(rs.choice([i for i, p in enumerate(PRICES) if p != o.price]))]
                offs.append(Offering(o.capacity_type, o.zone, price, bool(rs.rand() >= 0.15)))
            else:
                offs.append(Offering(cts[int(rs.randint(len(cts)))], zs[int(rs.randint(zones))], PRICES[int(rs.randint(len(PRICES)))], bool(rs.rand() >= 0.15)))
        cpu = 16 if t == types - 1 else int(rs.choice([2, 4, 8, 16]))
        its.append(fake.new_instance_type(f"pt-{t}", {"cpu": str(cpu), "memory": f"{2 * cpu}Gi", "pods": "32"}, offs))

    def selector():
        z, c = zs[-1] if rs.rand() < 0.25 else zs[int(rs.randint(zones))], cts[int(rs.randint(len(cts)))]
        some_z = [str(x) for x in rs.choice(zs, size=min(zones, int(rs.randint(1, 4))), replace=False)]
        some_c = [str(x) for x in rs.choice(list(cts), size=min(len(cts), int(rs.randint(1, 3))), replace=False)]
        return [[], [Expr(ZONE, "In", [z])], [Expr(ZONE, "In", some_z)], [Expr(ZONE, "NotIn", [z])], [Expr(CT, "In", [c])], [Expr(CT, "NotIn", [c])],
                [Expr(CT, "In", some_c)], [Expr(ZONE, "NotIn", some_z), Expr(CT, "In", [c])], [Expr(ZONE, "In", some_z), Expr(CT, "NotIn", [c])],
                [Expr(ZONE, "NotIn", [z]), Expr(CT, "NotIn", [c])]][int(rs.randint(10))]

    out = []
    for i in range(pods):
        sel = selector()
        out.append(Pod(uid=f"pp-{i:04d}", labels={"app": f"a{i % 3}"}, required_affinity=[sel] if sel else [],
                       containers=[Container(requests={"cpu": str(int(rs.choice([250, 500, 1000, 1500]))) + "m", "memory": "256Mi"})]))
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=out, extra_well_known=list(fake.EXTRA_WELL_KNOWN))


def _it(name, offerings):
    return fake.new_instance_type(name, {"cpu": "4", "memory": "8Gi", "pods": "32"}, [Offering(c, z, p, a) for c, z, p, a in offerings])


def _pod(uid, *exprs):
    return Pod(uid=uid, required_affinity=[list(exprs)] if exprs else [], containers=[Container(requests={"cpu": "500m", "memory": "256Mi"})])


def _problem(its, pods):
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=pods, extra_well_known=list(fake.EXTRA_WELL_KNOWN))


def duplicate_pairs():
    """dup-a repeats (z-a, spot) at 0.5 and 1.0 and (z-a, on-demand) at 0.25 and 3.0: worstLaunchPrice reads the maximum, Cheapest the minimum.
    Three pods whose selectors exclude each other: one new node per pod -- (z-a, spot), (z-a, on-demand), (z-b, on-demand)."""
    its = [_it("dup-a", [("spot", "z-a", 0.5, True), ("spot", "z-a", 1.0, True), ("on-demand", "z-a", 0.25, True), ("on-demand", "z-a", 3.0, True)]),
           _it("dup-b", [("spot", "z-a", 0.75, True), ("on-demand", "z-a", 0.75, True)]),
           _it("dup-c", [("on-demand", "z-a", 0.5, True), ("on-demand", "z-b", 1.5, True), ("on-demand", "z-b", 0.0, True)])]
    return _problem(its, [_pod("p-spot", Expr(CT, "In", ["spot"]), Expr(ZONE, "In", ["z-a"])),
                          _pod("p-od", Expr(CT, "In", ["on-demand"]), Expr(ZONE, "In", ["z-a"])),
                          _pod("p-zb", Expr(CT, "NotIn", ["spot"]), Expr(ZONE, "NotIn", ["z-a"]))])


def unavailable_offerings():
    """un-a's only available offering is (z-a, spot) at 1.0, beside unavailable ones above and below it on the same pair; un-b has no available spot offering
    (worstLaunchPrice falls through to on-demand), un-c nothing available at all (never an option)."""
    its = [_it("un-a", [("spot", "z-a", 3.0, False), ("spot", "z-a", 0.25, False), ("spot", "z-a", 1.0, True), ("on-demand", "z-a", 0.0, False)]),
           _it("un-b", [("spot", "z-a", 0.5, False), ("on-demand", "z-a", 0.75, True), ("on-demand", "z-a", 0.0, False)]),
           _it("un-c", [("spot", "z-a", 0.0, False), ("on-demand", "z-a", 0.0, False)])]
    return _problem(its, [_pod("p", Expr(ZONE, "In", ["z-a"]))])


def ties():
    """Three types whose cheapest offering is 0.5, 0.5 and 0.5000000000000001: the pick is the lower index of the two at 0.5 (tie-b, index 1), and a ceiling
    of 0.5 or of the next double decides between them."""
    its = [_it("tie-c", [("spot", "z-a", 0.5000000000000001, True)]), _it("tie-b", [("spot", "z-a", 0.5, True)]), _it("tie-a", [("spot", "z-a", 0.5, True)]),
           _it("tie-d", [("spot", "z-a", 0.0, False), ("spot", "z-a", 0.75, True)])]
    return _problem(its, [_pod("p", Expr(ZONE, "In", ["z-a"]))])


BUILDERS = {"catalogue": price_catalogue, "duplicate_pairs": duplicate_pairs, "unavailable_offerings": unavailable_offerings, "ties": ties}


def build_problem(spec):
    return BUILDERS[spec[0]](**spec[1])


# the stage cases: one Solve each, every new node through all three kernels
STAGE = {
    "spot_on_demand-1": ("catalogue", {"seed": 1}),
    "spot_on_demand-2": ("catalogue", {"seed": 2, "types": 48, "pods": 60}),
    "spot_on_demand-3": ("catalogue", {"seed": 3}),
    "third_capacity_type-11": ("catalogue", {"seed": 11, "cts": ("spot", "on-demand", "reserved")}),
    "third_capacity_type-12": ("catalogue", {"seed": 12, "cts": ("spot", "on-demand", "reserved"), "zones": 4}),
    "no_spot-21": ("catalogue", {"seed": 21, "cts": ("on-demand",)}),
    "no_spot-22": ("catalogue", {"seed": 22, "cts": ("on-demand",), "zones": 2}),
    "pairs_64-37": ("catalogue", {"seed": 37, "zones": 32, "types": 48, "pods": 60}),
    "pairs_64-39": ("catalogue", {"seed": 39, "zones": 32, "types": 48, "pods": 60}),
    "types_65-41": ("catalogue", {"seed": 41, "types": 65}),
    "types_65-42": ("catalogue", {"seed": 42, "types": 65, "pods": 60}),
    "tw_over_64-51": ("catalogue", {"seed": 51, "types": 4160, "pods": 24}),
    "duplicate_pairs": ("duplicate_pairs", {}),
    "unavailable_offerings": ("unavailable_offerings", {}),
    "ties": ("ties", {}),
}


# ---------------------------------------------------------------------------------------------------------------- the device side
def _price_filter_raw(S, flats, nodes, ceilings, spot_only):
    """ksh_price_filter with its count words: (kept type indices read from the WHOLE stride of each row -- a bit past the problem's own T or in the padding
    words shows up as an index >= T --, counts)."""
    import ctypes
    kh = S.libs()[1]
    n = len(flats)
    stride = max((f.dims["T"] + 63) // 64 for f in flats)
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    masks, counts = (ctypes.c_uint64 * (n * stride))(), (ctypes.c_uint32 * n)()
    so = (ctypes.c_uint32 * n)(*[1 if x else 0 for x in spot_only]) if spot_only is not None else None
    rc = kh.ksh_price_filter(hs, n, (ctypes.c_uint32 * n)(*nodes), (ctypes.c_double * n)(*ceilings), so, masks, stride, counts)
    if rc != S.KS_OK:
        raise S.KSolveError(rc, kh.ksh_last_error().decode())
    rows = [[w * 64 + b for w in range(stride) for b in range(64) if (masks[i * stride + w] >> b) & 1] for i in range(n)]
    return rows, [int(c) for c in counts]


def _universe(S, f, which):
    kh, out = S.libs()[1], []
    while kh.ksh_key_value(f._h, which, len(out)) is not None:
        out.append(kh.ksh_key_value(f._h, which, len(out)).decode())
    return out


def device_run(S, job):
    """Solve every problem of the job on its own handle, then make the job's calls, in order, on those handles.  Plain data in, plain data out (prices as
    float.hex, exact)."""
    flats = [S.FlatProblem(build_problem(spec)) for spec in job["problems"]]
    try:
        out = {"solves": [f.solve().canonical() for f in flats], "zones": [_universe(S, f, 0) for f in flats], "cts": [_universe(S, f, 1) for f in flats], "calls": []}
        for call in job["calls"]:
            at = call["at"]
            fl, nodes = [flats[e[0]] for e in at], [e[1] for e in at]
            if call["op"] == "pf":
                rows, counts = _price_filter_raw(S, fl, nodes, [float.fromhex(e[2]) for e in at], [e[3] for e in at] if call.get("spot") else None)
                out["calls"].append({"rows": rows, "counts": counts})
            elif call["op"] == "lp":
                out["calls"].append({"picks": [None if p is None else [p[0], p[1], p[2], float.hex(p[3])] for p in S.launch_pick(fl, nodes)]})
            else:
                out["calls"].append({"subset": S.types_subset(fl, nodes, [e[2] for e in at])})
        return out
    finally:
        for f in flats:
            f.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_price_stage as P
out = {}
for name, job in jobs["jobs"].items():
    try:
        out[name] = P.device_run(S, job)
    except Exception as e:
        out[name] = {"error": repr(e)[:300]}
print("RESULT " + json.dumps(out))
"""


def run_in_child(jobs, sim, tmp):
    """All `jobs` in ONE fresh process, in their order (a job's calls may depend on what the process did before: that is what the call-order case checks).
    A child that dies leaves every one of its jobs an error, which the tests that read them report."""
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    path = os.path.join(tmp, f"jobs_{len(os.listdir(tmp))}.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "jobs": jobs}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in jobs}
    return json.loads(line[-1][7:])


# ---------------------------------------------------------------------------------------------------------------- inputs and references
_REFS = {}


def reference(spec):
    """(problem, the oracle's Solve, type name -> index) of a case, built once per process."""
    key = json.dumps(spec, sort_keys=True)
    if key not in _REFS:
        pr = build_problem(spec)
        _REFS[key] = (pr, O.solve(pr), {it.name: t for t, it in enumerate(pr.instance_types)})
    return _REFS[key]


def node_reqs(node, spot_only):
    """The node's requirements; spot_only: Requirements.Add(capacity-type In [spot]) first -- In [spot] if the requirement admits spot, else In []."""
    reqs = dict(node.requirements)
    if spot_only:
        reqs[CT] = CR.Narrowed(["spot"] if CR.req_has(reqs.get(CT), "spot") else [])
    return reqs


def worst_prices(pr, node, spot_only):
    by_name = {it.name: it for it in pr.instance_types}
    return {n: CR.worst_launch_price(by_name[n].offerings, node_reqs(node, spot_only)) for n in node.instance_types}


def ceilings(pr, node, spot_only):
    """Every distinct worst price among the node's options (that type must drop: the compare is a strict <), the next double above each (it must come back),
    0.0, MaxFloat64 (a type with no admissible offering is priced exactly there and drops) and +inf."""
    worst = set(worst_prices(pr, node, spot_only).values())
    return sorted(worst | {math.nextafter(w, math.inf) for w in worst} | {0.0, CR.MAX_FLOAT64, math.inf})


def subset_sets(T, opts):
    """The empty set, the options, half of them, the options plus one outsider, and sets that straddle the 64-type words (and the 4096-type mark past which a
    lane owns a second word)."""
    outside = [t for t in range(T) if t not in set(opts)]
    sets = [[], list(opts), opts[: len(opts) // 2]]
    if outside:
        sets.append(sorted(opts + outside[:1]))
        sets.append(sorted(opts + outside[-1:]))
    for edge in (64, 128, 4096):
        if T > edge:
            lo, hi = [t for t in opts if t < edge][-2:], [t for t in opts if t >= edge][:2]
            sets.append(lo + hi)
            sets.append([edge - 1, edge])
            out_hi = [t for t in outside if t >= edge][:1]
            sets.append(sorted(lo + hi + out_hi))
    return sets


def stage_job(spec):
    """The calls of one stage case: price_filter at every ceiling without spot_only (no flag array at all), then with a flag per entry (both settings), the
    launch pick of every node, and the subset sets of every node."""
    pr, ref, idx = reference(spec)
    pf, pf_spot, lp, ts = [], [], [], []
    for j, node in enumerate(ref.new_nodes):
        pf += [(0, j, c.hex(), False) for c in ceilings(pr, node, False)]
        pf_spot += [(0, j, c.hex(), s) for s in (True, False) for c in ceilings(pr, node, s)]
        lp.append((0, j))
        ts += [(0, j, s) for s in subset_sets(len(pr.instance_types), [idx[n] for n in node.instance_types])]
    return {"problems": [spec], "calls": [{"op": "pf", "at": pf}, {"op": "pf", "spot": True, "at": pf_spot}, {"op": "lp", "at": lp}, {"op": "ts", "at": ts}]}


# one call over problems of different T (40, 65, 4160, 4, 40): the stride of a row is the largest TW, every problem's row sits at its own offset; nodes out of
# order and repeated
BATCH = ["spot_on_demand-1", "types_65-41", "tw_over_64-51", "ties", "third_capacity_type-11"]


def batch_job():
    rs = np.random.RandomState(7)
    pf, lp, ts = [], [], []
    for k, name in enumerate(BATCH):
        pr, ref, idx = reference(STAGE[name])
        for j, node in enumerate(ref.new_nodes):
            s = bool(rs.rand() < 0.5)
            pf += [(k, j, c.hex(), s) for c in ceilings(pr, node, s)]
            lp.append((k, j))
            ts += [(k, j, x) for x in subset_sets(len(pr.instance_types), [idx[n] for n in node.instance_types])]
    mix = lambda xs: [xs[i] for i in rs.permutation(len(xs))] + [xs[i] for i in rs.choice(len(xs), size=len(xs) // 3)]
    pf, lp, ts = mix(pf), mix(lp), mix(ts)
    assert any(a[0] == b[0] and a[1] > b[1] for a, b in zip(lp, lp[1:]))          # (out of order within a problem)
    return {"problems": [STAGE[n] for n in BATCH], "calls": [{"op": "pf", "spot": True, "at": pf}, {"op": "lp", "at": lp}, {"op": "ts", "at": ts}]}


# the call-order case: one sequence of calls on the same handles; every result must be the result of the same call made FIRST in a fresh process
SEQ_CASE = "spot_on_demand-2"
SEQUENCE = ["pf", "lp", "ts", "pf_spot", "lp", "pf"]


def sequence_calls():
    pr, ref, idx = reference(STAGE[SEQ_CASE])
    nodes = range(len(ref.new_nodes))
    return {"pf": {"op": "pf", "at": [(0, j, c.hex(), False) for j in nodes for c in ceilings(pr, ref.new_nodes[j], False)]},
            "pf_spot": {"op": "pf", "spot": True, "at": [(0, j, c.hex(), True) for j in nodes for c in ceilings(pr, ref.new_nodes[j], True)]},
            "lp": {"op": "lp", "at": [(0, j) for j in nodes]},
            "ts": {"op": "ts", "at": [(0, j, s) for j in nodes for s in subset_sets(len(pr.instance_types), [idx[n] for n in ref.new_nodes[j].instance_types])]}}


def all_results(sim, tmp):
    """Every case on one backend: the stage cases and the mixed-T batch in one process, the call sequence in another, each call of the sequence alone in a
    process of its own."""
    jobs = {name: stage_job(spec) for name, spec in STAGE.items()}
    jobs["batch"] = batch_job()
    out = {"stage": run_in_child(jobs, sim, tmp)}
    calls = sequence_calls()
    out["sequence"] = run_in_child({"sequence": {"problems": [STAGE[SEQ_CASE]], "calls": [calls[c] for c in SEQUENCE]}}, sim, tmp)["sequence"]
    out["first"] = {c: run_in_child({c: {"problems": [STAGE[SEQ_CASE]], "calls": [calls[c]]}}, sim, tmp)[c] for c in calls}
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return all_results(True, str(tmp_path_factory.mktemp("price_stage_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return all_results(bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("price_stage_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


# ---------------------------------------------------------------------------------------------------------------- checks
def checked_solves(got, specs):
    """The job's Solves on the device are the oracle's (so node j means the same node on both sides); -> the references."""
    assert "error" not in got, got
    refs = [reference(s) for s in specs]
    for k, (pr, ref, _) in enumerate(refs):
        assert json.loads(json.dumps(got["solves"][k])) == json.loads(json.dumps(ref.canonical())), k
        assert ref.new_nodes
    return refs


def check_price_filter(refs, call, got):
    assert len(got["rows"]) == len(got["counts"]) == len(call["at"])
    for e, row, count in zip(call["at"], got["rows"], got["counts"]):
        k, j, c, s = e
        pr, ref, idx = refs[k]
        node = ref.new_nodes[j]
        want = sorted(idx[n] for n in CR.filter_by_price({it.name: it for it in pr.instance_types}, node.instance_types, node_reqs(node, s), float.fromhex(c)))
        assert (row, count) == (want, len(want)), (e, row, count, want)


def check_launch_pick(refs, call, got):
    assert len(got["picks"]) == len(call["at"])
    for e, pick in zip(call["at"], got["picks"]):
        k, j = e
        pr, ref, idx = refs[k]
        node = ref.new_nodes[j]
        assert [idx[n] for n in node.instance_types] == sorted(idx[n] for n in node.instance_types)     # options in index order: CR's "earlier option" IS the lower index
        want = CR.launch_pick(pr.instance_types, node)
        if want is None:
            assert pick is None, e
            continue
        t, zone, ct, price = pick
        assert (pr.instance_types[t].name, price) == (want[0], float.hex(want[1])), (e, pick, want)       # bit for bit
        zr, cr = node.requirements.get(ZONE), node.requirements.get(CT)
        assert CR.req_has(zr, zone) and CR.req_has(cr, ct), (e, pick)
        assert any(o.available and (o.zone, o.capacity_type) == (zone, ct) and float.hex(o.price) == price for o in pr.instance_types[t].offerings), (e, pick)


def check_types_subset(refs, call, got):
    assert len(got["subset"]) == len(call["at"])
    for e, ok in zip(call["at"], got["subset"]):
        k, j, s = e
        pr, ref, _ = refs[k]
        assert ok == CR.instance_types_are_subset([pr.instance_types[t].name for t in s], ref.new_nodes[j].instance_types), (e, ok)


CHECKS = {"pf": check_price_filter, "lp": check_launch_pick, "ts": check_types_subset}


def _stage(res, name):
    job = stage_job(STAGE[name])
    got = res["stage"][name]
    return job, checked_solves(got, job["problems"]), got


def _ops(job, got, op):
    return [(c, g) for c, g in zip(job["calls"], got["calls"]) if c["op"] == op]


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(STAGE))
def test_price_filter_matches_filter_by_price(request, backend, case):
    """Every new node, every ceiling, with and without spot_only: the kept set and its count are filterByPrice's."""
    job, refs, got = _stage(request.getfixturevalue(backend), case)
    for call, g in _ops(job, got, "pf"):
        check_price_filter(refs, call, g)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(STAGE))
def test_launch_pick_matches_the_reference(request, backend, case):
    """Type and price bit for bit; the (zone, capacity type) is an available, admissible offering of that type at exactly that price."""
    job, refs, got = _stage(request.getfixturevalue(backend), case)
    for call, g in _ops(job, got, "lp"):
        check_launch_pick(refs, call, g)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(STAGE))
def test_types_subset_matches_the_reference(request, backend, case):
    job, refs, got = _stage(request.getfixturevalue(backend), case)
    for call, g in _ops(job, got, "ts"):
        check_types_subset(refs, call, g)


def _picks(res, name):
    return res["stage"][name]["calls"][2]["picks"]


def _rows(res, name, spot_only):
    """{(node, ceiling): kept type names} of a stage case's price_filter calls (spot_only False: the call without a flag array)."""
    job = stage_job(STAGE[name])
    pr = reference(STAGE[name])[0]
    call, got = (job["calls"][1], res["stage"][name]["calls"][1]) if spot_only else (job["calls"][0], res["stage"][name]["calls"][0])
    return {(e[1], float.fromhex(e[2])): {pr.instance_types[t].name for t in row} for e, row in zip(call["at"], got["rows"]) if e[3] == spot_only}


def _node_of_pod(ref, uid):
    pr, res, _ = ref
    return next(j for j, n in enumerate(res.new_nodes) if any(pr.pods[i].uid == uid for i in n.pods))


@pytest.mark.parametrize("backend", BACKENDS)
def test_duplicate_pairs_worst_price_is_the_maximum_and_cheapest_the_minimum(request, backend):
    """dup-a offers (z-a, spot) at 0.5 and 1.0: worstLaunchPrice is 1.0, the pick's price 0.5.  With the two encodings swapped the pick would be dup-b at 0.75
    and a ceiling of 1.0 would keep dup-a."""
    res = request.getfixturevalue(backend)
    job, refs, got = _stage(res, "duplicate_pairs")
    spot, od, zb = (_node_of_pod(refs[0], uid) for uid in ("p-spot", "p-od", "p-zb"))
    picks = _picks(res, "duplicate_pairs")
    assert [picks[j][:3] + [float.fromhex(picks[j][3])] for j in (spot, od, zb)] == [[0, "z-a", "spot", 0.5], [0, "z-a", "on-demand", 0.25], [2, "z-b", "on-demand", 0.0]]
    rows = _rows(res, "duplicate_pairs", False)
    assert rows[(spot, 1.0)] == {"dup-b"} and rows[(spot, math.nextafter(1.0, math.inf))] == {"dup-a", "dup-b"}
    assert rows[(od, 3.0)] == {"dup-b", "dup-c"} and rows[(zb, 1.5)] == set() and rows[(zb, math.nextafter(1.5, math.inf))] == {"dup-c"}


@pytest.mark.parametrize("backend", BACKENDS)
def test_unavailable_offerings_are_never_priced(request, backend):
    """un-a's unavailable (z-a, spot) offerings at 3.0 and 0.25 count neither for its worst price (1.0) nor for its cheapest (1.0); un-b has no available spot
    offering, so it is priced on-demand (0.75) -- and, priced as spot only, not at all (MaxFloat64); un-c is never an option."""
    res = request.getfixturevalue(backend)
    job, refs, got = _stage(res, "unavailable_offerings")
    node = refs[0][1].new_nodes[0]
    assert node.instance_types == ["un-a", "un-b"]
    assert [p[0] for p in _picks(res, "unavailable_offerings")] == [1] and float.fromhex(_picks(res, "unavailable_offerings")[0][3]) == 0.75
    rows, spot = _rows(res, "unavailable_offerings", False), _rows(res, "unavailable_offerings", True)
    assert rows[(0, 0.75)] == set() and rows[(0, 1.0)] == {"un-b"} and rows[(0, math.nextafter(1.0, math.inf))] == {"un-a", "un-b"}
    assert spot[(0, CR.MAX_FLOAT64)] == {"un-a"} and spot[(0, math.inf)] == {"un-a", "un-b"}


@pytest.mark.parametrize("backend", BACKENDS)
def test_ties_go_to_the_lowest_type_index(request, backend):
    """tie-b (index 1) and tie-a (index 2) both cost 0.5, tie-c (index 0) one ulp more: the pick is tie-b at exactly 0.5.  A ceiling of 0.5 keeps none of the
    three, the next double keeps the two at 0.5 and drops tie-c."""
    res = request.getfixturevalue(backend)
    _stage(res, "ties")
    assert _picks(res, "ties") == [[1, "z-a", "spot", float.hex(0.5)]]
    rows = _rows(res, "ties", False)
    assert rows[(0, 0.5)] == set() and rows[(0, 0.5000000000000001)] == {"tie-a", "tie-b"} and rows[(0, math.nextafter(0.5000000000000001, math.inf))] == {"tie-a", "tie-b", "tie-c"}
    ties = 0
    for name, spec in STAGE.items():         # the generated catalogues tie too: count the nodes whose cheapest price is shared by two options
        pr, ref, _ = reference(spec)
        by_name = {it.name: it for it in pr.instance_types}
        for node in ref.new_nodes:
            zr, cr = node.requirements.get(ZONE), node.requirements.get(CT)
            lows = [min([o.price for o in by_name[n].offerings if o.available and CR.req_has(zr, o.zone) and CR.req_has(cr, o.capacity_type)] or [math.inf]) for n in node.instance_types]
            ties += lows.count(min(lows)) > 1
    assert ties >= 5


@pytest.mark.parametrize("backend", BACKENDS)
def test_spot_only_prices_the_node_as_spot(request, backend):
    """consolidation.go:262-265: spot_only narrows the capacity-type requirement to In [spot] before pricing.  Checked against filterByPrice over the narrowed
    requirements above; here, that the flag changes answers at all, and that in a catalogue without spot it leaves nothing below MaxFloat64."""
    res = request.getfixturevalue(backend)
    changed = 0
    for name in STAGE:
        _stage(res, name)
        plain, spot = _rows(res, name, False), _rows(res, name, True)
        changed += sum(plain[k] != spot[k] for k in spot if k in plain)
        if name.startswith("no_spot"):
            assert all(not kept for (j, c), kept in spot.items() if c <= CR.MAX_FLOAT64)
    assert changed >= 10


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_ceiling_equal_to_a_worst_price_drops_it_and_one_ulp_above_keeps_it(request, backend):
    """filterByPrice keeps `worst < price`: at every option's own worst price that option is out, at the next double it is in -- also where a float32 or a
    fused compare would merge 0.5 and 0.5000000000000001."""
    res = request.getfixturevalue(backend)
    seen_ulp = 0
    for name, spec in STAGE.items():
        _stage(res, name)
        pr, ref, _ = reference(spec)
        for spot_only in (False, True):
            rows = _rows(res, name, spot_only)
            for j, node in enumerate(ref.new_nodes):
                worst = worst_prices(pr, node, spot_only)
                for n, w in worst.items():
                    assert n not in rows[(j, w)] and (n in rows[(j, math.nextafter(w, math.inf))]), (name, j, n, w, spot_only)
                seen_ulp += {0.5, 0.5000000000000001} <= set(worst.values())
    assert seen_ulp >= 3


def _universe_of(res, name):
    got = res["stage"][name]
    return got["zones"][0], got["cts"][0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_no_spot_catalogue(request, backend):
    """ct_spot < 0: no capacity type called spot anywhere; worstLaunchPrice goes straight to on-demand."""
    res = request.getfixturevalue(backend)
    for name in ("no_spot-21", "no_spot-22"):
        _stage(res, name)
        assert _universe_of(res, name)[1] == ["on-demand"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_third_capacity_type(request, backend):
    """`reserved` is priced by neither branch of worstLaunchPrice (MaxFloat64 when it is all a node admits) but is an offering like any other for the pick."""
    res = request.getfixturevalue(backend)
    picked = set()
    for name in ("third_capacity_type-11", "third_capacity_type-12"):
        _stage(res, name)
        assert sorted(_universe_of(res, name)[1]) == ["on-demand", "reserved", "spot"]
        picked |= {p[2] for p in _picks(res, name) if p}
    assert "reserved" in picked


def _covers_pair(pr, ref, idx, zones, cts, pair):
    z, c = zones[pair // len(cts)], cts[pair % len(cts)]
    for node in ref.new_nodes:
        zr, cr = node.requirements.get(ZONE), node.requirements.get(CT)
        if CR.req_has(zr, z) and CR.req_has(cr, c) and any(o.available and (o.zone, o.capacity_type) == (z, c) for n in node.instance_types for o in pr.instance_types[idx[n]].offerings):
            return True
    return False


@pytest.mark.parametrize("backend", BACKENDS)
def test_pairs_64(request, backend):
    """32 zones x 2 capacity types: the offering bitmask is full and pair 63 (the last zone's second capacity type) is admissible on some new node."""
    res = request.getfixturevalue(backend)
    covered = False
    for name in ("pairs_64-37", "pairs_64-39"):
        _stage(res, name)
        zones, cts = _universe_of(res, name)
        assert len(zones) * len(cts) == 64
        pr, ref, idx = reference(STAGE[name])
        covered |= _covers_pair(pr, ref, idx, zones, cts, 63)
    assert covered


@pytest.mark.parametrize("backend", BACKENDS)
def test_types_65_and_tw_over_64(request, backend):
    """T = 65 (type 64 is bit 0 of word 1) and T = 4160 (TW = 65 > 64: lane 0 walks words 0 and 64): some node's options sit on both sides of the edge."""
    res = request.getfixturevalue(backend)
    for name, edge in (("types_65-41", 64), ("types_65-42", 64), ("tw_over_64-51", 4096)):
        _stage(res, name)
        pr, ref, idx = reference(STAGE[name])
        assert any(min(idx[n] for n in nd.instance_types) < edge <= max(idx[n] for n in nd.instance_types) for nd in ref.new_nodes), name


@pytest.mark.parametrize("backend", BACKENDS)
def test_batch_of_mixed_t(request, backend):
    """One call over problems with T = 40, 65, 4160, 4 and 40 (TW 1, 2, 65, 1, 1; the stride is 65 words), nodes out of order and repeated: each entry is
    its own problem's answer, nothing lands in another's row or in the padding."""
    res = request.getfixturevalue(backend)
    job, got = batch_job(), res["stage"]["batch"]
    refs = checked_solves(got, job["problems"])
    assert sorted({len(r[0].instance_types) for r in refs}) == [4, 40, 65, 4160]
    for call, g in zip(job["calls"], got["calls"]):
        CHECKS[call["op"]](refs, call, g)


@pytest.mark.parametrize("backend", BACKENDS)
def test_call_order_does_not_change_results(request, backend):
    """price_filter, launch_pick, types_subset, price_filter with spot_only, launch_pick, price_filter on the same handles: each result is the result of the
    same call made first in a fresh process (and the reference's).  Device temporaries that were handed back to the pool more than once broke this."""
    res = request.getfixturevalue(backend)
    calls = sequence_calls()
    seq = res["sequence"]
    refs = checked_solves(seq, [STAGE[SEQ_CASE]])
    assert len(seq["calls"]) == len(SEQUENCE)
    for step, (c, got) in enumerate(zip(SEQUENCE, seq["calls"])):
        first = res["first"][c]
        checked_solves(first, [STAGE[SEQ_CASE]])
        assert got == first["calls"][0], (step, c)
        CHECKS[calls[c]["op"]](refs, calls[c], got)


def test_the_catalogues_have_the_edges():
    """(CPU) The generator makes what the cases above are named after: repeated pairs at different prices, about 15 % unavailable offerings, both doubles
    around 0.5 and 0.0."""
    offers = [o for spec in STAGE.values() if spec[0] == "catalogue" for it in build_problem(spec).instance_types for o in it.offerings]
    assert 0.08 < sum(not o.available for o in offers) / len(offers) < 0.25
    assert {0.0, 0.5, 0.5000000000000001} <= {o.price for o in offers}
    dup = 0
    for spec in STAGE.values():
        for it in build_problem(spec).instance_types:
            seen = {}
            for o in it.offerings:
                seen.setdefault((o.zone, o.capacity_type), set()).add(o.price)
            dup += any(len(p) > 1 for p in seen.values())
    assert dup >= 100
