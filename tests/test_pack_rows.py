"""Every ks_pack instantiation (karpenter_core_amd/csrc/ksolve.hip: pack_rows) against the oracle, on both sides of the limits that decide which one runs.

The reference is oracle_py.solve, never the product: every run compares canonical() and reasons with the oracle's result of the same problem.  Every run also
asserts `FlatProblem.pack_row()` -- the row ks_solve_batch_dev launched (ks_problem_pack_row) -- so a case that lands on another body fails instead of passing
for the wrong reason.  A case is one problem and several runs of it: each run names how the row is reached -- one Solve or a batch of two independent problems,
and the flags of the problem (KS_FLAG_NO_RR always: ks_pack_rr has its own files; KS_FLAG_ONE_WAVE / KS_FLAG_NO_LEAN / KS_FLAG_STATS) -- and the row fields
(FAST, BOUNDS, LEAN, NW, RM) it was written for.  Where a flag can reach a different row the case runs under both; the single-wave general rows (0..3) and the
wide rows (12..15) are fixed points of the flags (never LEAN, never multi-wave once asked for one wave), so those cases run a second time as a batch, which
launches the same row over a grid of two with the batch's 64 KiB of dynamic LDS.

The limits (ks_solve_batch_dev's FAST test, pack_choose's LADDERS44 / TW128, and the bodies' own: ls.hslot_of[64], the g & 63 mask bits, hs < 24 / GH <= 24,
dyn_groups' 16 groups and 8 values), each with a case just inside and one just outside:
  G 64 | 65 (and 70: six groups past 63, zonal and hostname-keyed alternating)      GH 64 | 65      GH 24 | 25 (the hostname dynamic rule of the multi-wave rows)
  S * SC 256 | 272      R * ge_max 6144 | 6147      R * ge_max 4608 | 4611 (multi-wave | single-wave FAST)      dynamic spread groups 16 | 17, key values 8 | 9
  T 8192 | 8193 (TW 128 | 129)
S * SC: SC is 1 + the number of distinct pod-side requirements on node.kubernetes.io/instance-type, S the closure of the node-side ones under intersection with
them (ksh_dims gives S, not SC).  Fifteen nested In-lists over a 16-type catalogue close to themselves: S = 16 (with the absent state), SC = 16, 256.  With SC = 16
every reachable product is a multiple of 16; the first above 256 is 272: one existing node carrying the instance-type label of the innermost list adds the one
state In [that type] (found by trying both: the labelled node gives dims S = 17 and a non-FAST row, the unlabelled ones S = 16 and a FAST row).

The emulator (KS_TEST_SIM=1) runs the single-wave rows; runs written for the four multi-wave rows skip there with that reason and run on the GPU."""
import functools
import json
import os
import subprocess
import sys

import pytest

from karpenter_core_amd import fake, scheduler as S
from karpenter_core_amd.model import (Container, Expr, HostPort, LabelSelector, Pod, PodAffinityTerm, Problem, StateNode, TopologySpreadConstraint,
                                      LABEL_ARCH, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_OS, LABEL_PROVISIONER, LABEL_ZONE, Offering)
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SIM = bool(os.environ.get("KS_TEST_SIM"))
NO_RR, ONE_WAVE, NO_LEAN, STATS = S.KS_FLAG_NO_RR, S.KS_FLAG_ONE_WAVE, S.KS_FLAG_NO_LEAN, S.KS_FLAG_STATS
DEVICE_NAMES = ["ephemeral-storage", "example.com/dev"]                                                     # requested: 5 active names
INERT_NAMES = ["example.com/a", "example.com/b", "example.com/c", "example.com/d", "example.com/e"]         # listed by the catalogue only: 10 names in all


# ------------------------------------------------------------------------------------------------ problems
def _types(n, zones, names, distinct_memory):
    """n instance types.  Sizes cycle over eight (cpu, memory, pods) shapes; distinct_memory: memory grows by 16Mi per type instead, so that Allocatable memory
    takes n pairwise distinct values (ge_max = n)."""
    shapes = [(2, 4, 4), (4, 8, 6), (8, 16, 10), (16, 32, 16), (4, 32, 8), (2, 8, 5), (8, 8, 7), (32, 64, 24)]
    zs = [f"test-zone-{z + 1}" for z in range(zones)]
    out = []
    for i in range(n):
        cpu, mem, pods = shapes[i % len(shapes)]
        res = {"cpu": str(cpu), "memory": f"{1024 + 16 * i}Mi" if distinct_memory else f"{mem}Gi", "pods": str(pods)}
        if names >= 5:
            res.update({"ephemeral-storage": f"{20 * (1 + i % 3)}Gi", "example.com/dev": str(i % 3)})
        if names >= 10:
            res.update({k: str((i + j) % 2) for j, k in enumerate(INERT_NAMES)})
        price = fake.price_from_resources(res) * (1 + i // len(shapes) * 1e-4)
        offs = [Offering(ct, z, price * (0.7 if ct == "spot" else 1.0)) for z in zs for ct in ("spot", "on-demand")]
        out.append(fake.new_instance_type(f"t{i:04d}", res, offs, "amd64", ["linux"]))
    return out


def build(kinds, types=8, zones=3, names=3, general=False, bounds=False, it_chain=0, label_nodes=True, distinct_memory=False, per=3, fillers=6, nodes=3):
    """One provisioning Solve.  `kinds`: one deployment per letter, in pod order -- which is the order its topology groups are created in --
    z: zonal spread (one group), h: hostname spread (one hostname-keyed group), a: required hostname anti-affinity (one hostname-keyed group and, after every
    other group, one hostname-keyed inverse group).  Every deployment owns its selector and has `per` pods (an anti-affinity one two), so counters move; requests
    differ between deployments, so the queue interleaves them.  `nodes` existing nodes with room for a few pods each, `fillers` pods without topology, one pod
    that fits nothing.  general: host ports on deployment 1 and a provisioner limit; bounds: Gt / Lt on the `integer` label of deployments 0 and 2;
    names 5: requests on ephemeral-storage and a device, 10: five more names only the catalogue lists; it_chain: deployment j < it_chain selects the instance
    types j.. (nested In-lists: distinct pod-side columns, and node filters of the zonal groups); label_nodes: the existing nodes carry the instance-type label."""
    its = _types(types, zones, names, distinct_memory)
    assert it_chain < types
    prov = fake.provisioner("default", len(its), limits={"cpu": "100000"} if general else None)
    sn = []
    for e in range(nodes):
        it = its[len(its) - 1 if it_chain else 1]
        name = f"rows-node-{e}"
        labels = {LABEL_PROVISIONER: "default", LABEL_ZONE: f"test-zone-{e % zones + 1}", LABEL_CAPACITY_TYPE: "on-demand", LABEL_ARCH: "amd64", LABEL_OS: "linux",
                  LABEL_HOSTNAME: name, "karpenter.sh/initialized": "true"}
        if label_nodes and (not it_chain or e == 0):
            labels[LABEL_INSTANCE_TYPE] = it.name
        avail = {"cpu": "1500m", "memory": "3Gi", "pods": "3"}
        if names >= 5:
            avail.update({"ephemeral-storage": "8Gi", "example.com/dev": "1"})
        sn.append(StateNode(name=name, labels=labels, available=avail, capacity=dict(it.capacity)))
    pods = []
    for d, kind in enumerate(kinds):
        sel = LabelSelector({"app": f"d{d}"})
        for k in range(2 if kind == "a" else per):
            c = Container(requests={"cpu": f"{250 + 125 * (d % 5)}m", "memory": f"{128 * (1 + d % 3)}Mi"})
            p = Pod(uid=f"d{d:03d}-{k}", labels={"app": f"d{d}"}, containers=[c])
            if kind == "z":
                p.spread = [TopologySpreadConstraint(1, LABEL_ZONE, label_selector=sel)]
            elif kind == "h":
                p.spread = [TopologySpreadConstraint(1, LABEL_HOSTNAME, label_selector=sel)]
            else:
                p.anti_required = [PodAffinityTerm(LABEL_HOSTNAME, sel)]
            if general and d == 1:
                c.ports = [HostPort(8080)]
            if bounds and d in (0, 2):
                p.required_affinity = [[Expr(fake.LABEL_INTEGER, "Gt", ["3"]) if d == 0 else Expr(fake.LABEL_INTEGER, "Lt", ["9"])]]
            if names >= 5 and d % 4 == 1:
                c.requests["ephemeral-storage"] = "2Gi"
            if names >= 5 and d % 4 == 3:
                c.limits["example.com/dev"] = "1"
            if d < it_chain:
                p.node_selector = {}
                p.required_affinity = [(p.required_affinity[0] if p.required_affinity else []) + [Expr(LABEL_INSTANCE_TYPE, "In", [t.name for t in its[d:]])]]
            pods.append(p)
    for k in range(fillers):
        pods.append(Pod(uid=f"fill-{k}", containers=[Container(requests={"cpu": f"{300 + 100 * k}m", "memory": "200Mi"})]))
    pods.append(Pod(uid="too-big", containers=[Container(requests={"cpu": "500", "memory": "1Gi"})]))
    return Problem(instance_types=its, provisioners=[prov], pods=pods, nodes=sn, extra_well_known=fake.EXTRA_WELL_KNOWN)


def _mix(z, h=0, a=0):
    """z zonal, h hostname-spread and a anti-affinity deployments; the hostname-keyed ones spread over the order, one of them last."""
    n = z + h + a
    marks = ["z"] * n
    slots = [n - 1 - i * max(1, n // max(1, h + a)) for i in range(h + a)]
    for i, s in enumerate(slots):
        marks[s] = "h" if i < h else "a"
    assert marks.count("z") == z
    return "".join(marks)


# ------------------------------------------------------------------------------------------------ cases
# row fields (FAST, BOUNDS, LEAN, NW, RM); the library's table (pack_rows) in its order, restated: the CPU test below compares
ROWS = [(f, b, l, 1, rm) for l, rm in ((0, 8), (1, 4), (1, 8), (0, 16)) for f in (0, 1) for b in (0, 1)] + [(1, 0, 1, 8, 4), (1, 0, 1, 4, 8), (1, 0, 0, 4, 8), (1, 1, 0, 4, 8)]


def _runs(fast, bounds, feature):
    """The runs of one problem of the G family, by what it is: feature lean / general / lean8 / wide."""
    f, b = int(fast), int(bounds)
    if feature == "wide":
        return [("single", "single", 0, (f, b, 0, 1, 16)), ("batch", "batch", 0, (f, b, 0, 1, 16))]
    if feature == "general":
        multi = [("multi", "single", 0, (1, b, 0, 4, 8))] if fast else []
        return multi + [("one_wave", "single", ONE_WAVE, (f, b, 0, 1, 8)), ("batch", "batch", 0, (f, b, 0, 1, 8))]
    rm = 8 if feature == "lean8" else 4
    multi = []
    if fast:
        multi = [("multi", "single", 0, (1, 1, 0, 4, 8) if bounds else (1, 0, 1, 8 if rm == 4 else 4, rm))]      # (LEAN with bounds: the general four waves)
    return multi + [("one_wave", "single", ONE_WAVE, (f, b, 1, 1, rm)), ("no_lean", "single", ONE_WAVE | NO_LEAN, (f, b, 0, 1, 8)), ("batch", "batch", 0, (f, b, 1, 1, rm)),
                    ("stats", "single", STATS, (f, b, 0, 1, 8))]


CASES = {}      # id -> (builder, active_resources, dims the flat problem must have, runs)


def _case(cid, builder, runs, active=False, **dims):
    CASES[cid] = (builder, active, dims, runs)


for _g, _fast in ((64, True), (65, False)):
    for _feature, _kw, _active in (("lean", {}, False), ("general", {"general": True}, False), ("lean8", {"names": 5}, True), ("wide", {"names": 10}, False)):
        for _b in (False, True):
            _case(f"g{_g}_{_feature}{'_bounds' if _b else ''}", functools.partial(build, _mix(_g - 12, 6, 3), bounds=_b, **_kw), _runs(_fast, _b, _feature), active=_active, G=_g,
                  R={"lean": 3, "general": 3, "lean8": 5, "wide": 10}[_feature])
_case("g70_lean", functools.partial(build, "z" * 58 + "zhzhzhzhzhzh"), _runs(False, False, "lean"), G=70, GH=6)
_case("gh64_lean", functools.partial(build, _mix(0, 24, 20), per=2, fillers=3), _runs(True, False, "lean"), G=64, GH=64)
_case("gh65_lean", functools.partial(build, _mix(0, 25, 20), per=2, fillers=3), _runs(False, False, "lean"), G=65, GH=65)
_case("gh24_lean", functools.partial(build, _mix(6, 8, 8)), _runs(True, False, "lean"), GH=24)
_case("gh25_lean", functools.partial(build, _mix(6, 9, 8)), _runs(True, False, "lean"), GH=25)
_case("ssc256_general", functools.partial(build, _mix(18, 2, 0), types=16, it_chain=15, label_nodes=False), _runs(True, False, "general"), S=16)
_case("ssc272_general", functools.partial(build, _mix(18, 2, 0), types=16, it_chain=15, label_nodes=True), _runs(False, False, "general"), S=17)
_case("rt6144_lean", functools.partial(build, _mix(8, 2, 1), types=2048, distinct_memory=True), [("single", "single", 0, (1, 0, 1, 1, 4)), ("no_lean", "single", NO_LEAN, (1, 0, 0, 1, 8))], T=2048)
_case("rt6147_lean", functools.partial(build, _mix(8, 2, 1), types=2049, distinct_memory=True), [("single", "single", 0, (0, 0, 1, 1, 4)), ("no_lean", "single", NO_LEAN, (0, 0, 0, 1, 8))], T=2049)
_case("rt4608_lean", functools.partial(build, _mix(8, 2, 1), types=1536, distinct_memory=True),
      [("multi", "single", 0, (1, 0, 1, 8, 4)), ("multi_no_lean", "single", NO_LEAN, (1, 0, 0, 4, 8)), ("one_wave", "single", ONE_WAVE, (1, 0, 1, 1, 4))], T=1536)
_case("rt4611_lean", functools.partial(build, _mix(8, 2, 1), types=1537, distinct_memory=True), [("single", "single", 0, (1, 0, 1, 1, 4)), ("no_lean", "single", NO_LEAN, (1, 0, 0, 1, 8))], T=1537)
_DYN = [("multi", "single", 0, (1, 0, 1, 8, 4)), ("multi_no_lean", "single", NO_LEAN, (1, 0, 0, 4, 8)), ("one_wave", "single", ONE_WAVE, (1, 0, 1, 1, 4)), ("no_lean", "single", ONE_WAVE | NO_LEAN, (1, 0, 0, 1, 8))]
_case("dyn16_groups", functools.partial(build, "z" * 16, per=4), _DYN, G=16)
_case("dyn17_groups", functools.partial(build, "z" * 17, per=4), _DYN, G=17)
_case("dyn8_values", functools.partial(build, "z" * 10, zones=8, per=9, nodes=4), _DYN, G=10)
_case("dyn9_values", functools.partial(build, "z" * 10, zones=9, per=10, nodes=4), _DYN, G=10)
_case("t8192_lean", functools.partial(build, _mix(6, 1, 1), types=8192, zones=2, fillers=3), [("multi", "single", 0, (1, 0, 1, 8, 4)), ("one_wave", "single", ONE_WAVE, (1, 0, 1, 1, 4))], T=8192)
_case("t8193_lean", functools.partial(build, _mix(6, 1, 1), types=8193, zones=2, fillers=3), [("single", "single", 0, (1, 0, 1, 1, 4)), ("no_lean", "single", NO_LEAN, (1, 0, 0, 1, 8))], T=8193)

EXPECTED = {f"{cid}-{run[0]}": run[3] for cid, (_, _, _, runs) in CASES.items() for run in runs}      # run id -> the row fields it was written for


# ------------------------------------------------------------------------------------------------ the oracle's side, once per case
@functools.lru_cache(maxsize=None)
def _reference(cid):
    """(problem, the oracle's result, a companion problem for the batch runs -- the same cluster with the last deployment's pods left out -- and its result);
    the properties that make the limit matter are asserted here, on the ORACLE's result."""
    builder = CASES[cid][0]
    pr = builder()
    want = O.solve(pr)
    assert len(want.new_nodes) >= 2, "the pods must open at least two nodes"
    assert any(want.existing.values()), "an existing node must take something (and refuse the rest: nodes were opened)"
    assert want.unscheduled and all(want.reasons.get(i, 0) != 0 for i in want.unscheduled), "a pod must end unschedulable, with a reason"
    small = None
    if any(run[1] == "batch" for run in CASES[cid][3]):
        sp = builder()
        last = [p.labels["app"] for p in sp.pods if "app" in p.labels][-1]
        sp.pods = [p for p in sp.pods if p.labels.get("app") != last]
        small = (sp, O.solve(sp))
    return pr, want, small


def _same(got, want, what):
    assert got.canonical() == want.canonical(), what
    assert got.reasons == want.reasons, what


@pytest.mark.gpu
@pytest.mark.parametrize("rid", sorted(EXPECTED))
def test_row_against_the_oracle(rid):
    cid, run = rid.rsplit("-", 1)
    builder, active, dims, runs = CASES[cid]
    _, mode, flags, fields = next(r for r in runs if r[0] == run)
    if SIM and fields[3] > 1:
        pytest.skip("a multi-wave row: the emulator runs ks_pack's single-wave instantiations only")
    pr, want, small = _reference(cid)
    flats = [S.FlatProblem(pr, flags=flags | NO_RR, active_resources=active)]
    try:
        for k, v in dims.items():
            assert flats[0].dims[k] == v, (k, flats[0].dims)
        if mode == "batch":
            flats.append(S.FlatProblem(small[0], flags=flags | NO_RR, active_resources=active))
            S.upload_batch(flats)
            got, _, _ = S.solve_batch(flats)
            wants = [want, small[1]]
        else:
            got, wants = [flats[0].solve()], [want]
        for f in flats:
            assert f.rr_status()[0] is False
            row = f.pack_row()
            assert row is not None and tuple(int(x) for x in row[1:]) == fields, (rid, row, fields)
            assert ROWS[row[0]] == fields and f.pack_width() == fields[4] and f.pack_lean() == bool(fields[2])
        for i, (g, w) in enumerate(zip(got, wants)):
            _same(g, w, (rid, i))
    finally:
        for f in flats:
            f.close()


@pytest.mark.gpu
def test_pack_row_says_when_ks_pack_did_not_run():
    """-1 (None) before any solve and after a Solve ks_pack_rr took; the row again once ks_pack takes the same problem."""
    pr, want, _ = _reference("dyn16_groups")
    f = S.FlatProblem(pr)
    try:
        f.upload()
        assert f.pack_row() is None
        got = f.solve()
        started, why = f.rr_status()
        assert (f.pack_row() is None) == (started and why == 0)
        _same(got, want, "ks_pack_rr or its fallback")
    finally:
        f.close()


# ------------------------------------------------------------------------------------------------ CPU: the cases cover the table
CHILD = r"""
import ctypes, json, sys
ks = ctypes.CDLL(sys.argv[1])
ks.ks_debug_pack_row.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
f = (ctypes.c_int32 * 6)()
n = ks.ks_debug_pack_row(0xFFFFFFFF, f)
table = []
for i in range(n):
    ks.ks_debug_pack_row(i, f)
    table.append(list(f)[:5])
json.dump(table, sys.stdout)
"""


def test_the_cases_cover_every_row_of_the_library():
    """The library's own row table (loaded in a child process, so this process keeps the libraries it has) against the expected rows of the cases: all 20 rows
    are some run's expected row, the four multi-wave ones included, and every expected row exists."""
    import __graft_entry__ as ge
    ge.build()
    pr = subprocess.run([sys.executable, "-c", CHILD, os.path.join(ROOT, "karpenter_core_amd", "libksolve.so")], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr
    table = [tuple(r) for r in json.loads(pr.stdout)]
    assert len(table) == 20 and table == ROWS
    wanted = set(EXPECTED.values())
    assert wanted <= set(table), wanted - set(table)
    assert set(table) <= wanted, f"rows no case is written for: {sorted(set(table) - wanted)}"
    assert sum(1 for r in table if r[3] > 1) == 4 and all(any(v == r for v in EXPECTED.values()) for r in table if r[3] > 1)
