"""include/ksolve.h names the arrays of `ks_problem` ONCE (`KS_PROBLEM_ARRAYS`): libkshost's flattening wires and checks them from the table, libksolve's upload copies
them from it, the fingerprint hashes them from it.  `ks_debug_problem_array` shows the table to a caller, and these tests walk it -- they keep no list of their own:

  1. the rows' pointer slots are distinct, 8-byte aligned, inside the struct, and with the scalars (the one list below) leave no slot of the struct uncovered;
  2. the names are unique, and exactly one row is marked as not fingerprinted;
  3. a problem REBUILT from exact-length copies -- every array in a buffer of exactly count * elem_bytes, an array of no elements passed as NULL -- solves to the
     bytes the original handle's arrays solve to, and to the oracle's result: no kernel and no upload reads an element the table does not count;
  4. a byte flipped in any fingerprinted array moves `ksh_fingerprint`; one flipped in `it_price_lo` does not.  (The byte is flipped in place, through the pointer
     `ksh_problem` shows -- the vector the fingerprint reads.)

The problems are a handful of pods and nodes each; together they give every row at least one element.  The kernels run in a child process: on the emulator build
(tests/sim) here, on the device in tests/test_problem_arrays_gpu.py."""
import ctypes
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np

from karpenter_core_amd import workloads as W
from karpenter_core_amd.model import (DO_NOT_SCHEDULE, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_ZONE, HostPort, LabelSelector, TopologySpreadConstraint, Volume)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# The scalar members of ks_problem (include/ksolve.h), four bytes each, by byte offset, and the padding after n_ct and after each ks_reqsets' n.  Everything else in the struct is a pointer a row names.
SCALARS = {"P": 0, "C": 4, "T": 8, "M": 12, "E": 16, "K": 20, "R": 24, "G": 28, "GH": 32, "S": 36, "SC": 40, "max_new_nodes": 44, "flags": 48, "wellknown_mask": 52,
           "key_zone": 72, "key_ct": 76, "n_ct": 80, "ct_spot": 152, "ct_ondemand": 156, "tmpl.n": 192, "en.n": 296, "ND": 392, "SW": 396, "cls.n": 424,
           "flt.n": 688, "n_topologies": 776, "lean_r8": 780}
PADDING = [84, 196, 300, 428, 692]
SIZEOF = 784
NOT_FINGERPRINTED, NULLABLE = 1, 2


# ---------------------------------------------------------------------------------------------------------------- the problems
def _cluster(seed, spare=2, existing=4, per_node=3):
    its, prov, nodes, bound = W.cluster_snapshot(existing, 4, seed, spare_pod_slots=spare)
    return its, prov, nodes, [b[:per_node] for b in bound]


def _ports_cluster():
    """Node 1 holds port 9000 for a pod of its own; the first pod of node 0 (the candidate) wants 9000 too, and 9001."""
    its, prov, nodes, bound = _cluster(15)
    assert bound[0] and bound[1]
    bound[1][0].containers[0].ports = [HostPort(port=9000)]
    nodes[1].host_ports = [HostPort(port=9000)]
    bound[0][0].containers[0].ports = [HostPort(port=9000), HostPort(port=9001)]
    nodes[0].host_ports = [HostPort(port=9000), HostPort(port=9001)]
    return its, prov, nodes, bound


def build_case(name):
    if name == "r3":
        return W.whatif(*_cluster(11), [0], False)
    if name == "r9":               # nine resource names: the wide kernels
        return W.wide_catalogue(names=9, pods=8, types=24, existing=4, seed=1)
    if name == "ports":
        return W.whatif(*_ports_cluster(), [0], False)
    if name == "ports_no_pods":    # P = 0, C = 0: `ports` is then as long as en_port_off says
        return dataclasses.replace(W.whatif(*_ports_cluster(), [0], False), pods=[])
    if name == "volumes":          # one CSI driver with a limit; claim "shared" is on node 1 before the candidate's pod, which mounts it too, arrives
        its, prov, nodes, bound = _cluster(13)
        for n in nodes:
            n.volume_limits = {W.EBS_DRIVER: 3}
        bound[1][0].volumes = nodes[1].volumes = [Volume(W.EBS_DRIVER, "default/shared")]
        bound[0][0].volumes = nodes[0].volumes = [Volume(W.EBS_DRIVER, "default/shared"), Volume(W.EBS_DRIVER, "default/own")]
        return W.whatif(its, prov, nodes, bound, [0], True)
    if name == "filter":           # a zonal spread group whose owner carries a node selector: one node-filter term
        its, prov, nodes, bound = _cluster(12)
        for p in bound[0][:2]:
            p.labels = {"my-label": "a"}
            p.node_selector = {LABEL_ZONE: nodes[1].labels[LABEL_ZONE]}
            p.spread = [TopologySpreadConstraint(1, LABEL_ZONE, DO_NOT_SCHEDULE, LabelSelector({"my-label": "a"}))]
        return W.whatif(its, prov, nodes, bound, [0], True)
    if name == "anti":             # hostname anti-affinity
        its, prov, nodes, bound = _cluster(14)
        rs = np.random.RandomState(14)
        bound[0] = [W.anti_affinity_pod(rs, f"anti-{i}", LABEL_HOSTNAME) for i in range(3)]
        return W.whatif(its, prov, nodes, bound, [0], True)
    if name == "it_in":            # a pod that names an instance type: states and columns of the instance-type key
        its, prov, nodes, bound = _cluster(16)
        bound[0][0].node_selector = {LABEL_INSTANCE_TYPE: its[-1].name}
        if len(bound[0]) > 1:      # and one that names a node: the hostname lists
            bound[0][1].node_selector = {LABEL_HOSTNAME: nodes[1].name}
        return W.whatif(its, prov, nodes, bound, [0], False)
    raise KeyError(name)


CASES = ["r3", "r9", "ports", "ports_no_pods", "volumes", "filter", "anti", "it_in"]
VARIANTS = CASES + ["r3/no_prices"]      # the same problem with it_price and it_price_lo NULL, as tests/cabi_usage_commands.c makes one


def shared_snapshot():
    """6 nodes, two candidate sets: what-ifs flattened over ONE snapshot share its catalogue and lattice arrays (ks_problem_upload_shared)."""
    its, prov, nodes, bound = _cluster(11, existing=6)
    snap, pod_node = W.snapshot_problem(its, prov, nodes, bound, False)
    sets = [[0], [1, 2]]
    return snap, pod_node, sets, [W.whatif(its, prov, nodes, bound, cs, False) for cs in sets]


# ---------------------------------------------------------------------------------------------------------------- the part that runs the kernels (child process)
class _Result(ctypes.Structure):      # include/ksolve.h ks_result
    _fields_ = [("pod_node", ctypes.c_void_p), ("pod_stage", ctypes.c_void_p), ("pod_seq", ctypes.c_void_p), ("pod_reason", ctypes.c_void_p), ("n_unscheduled", ctypes.c_uint32),
                ("unscheduled", ctypes.c_void_p), ("n_new", ctypes.c_uint32)] + \
               [(n, ctypes.c_void_p) for n in ("node_tmpl", "node_types", "node_requests", "node_requests_present", "node_present", "node_complement", "node_mask", "node_gt",
                                               "node_lt", "node_it_state")] + [("stats", ctypes.c_uint64 * 32)]


def _u32(raw, off):
    return int.from_bytes(raw[off:off + 4], "little")


def rows_of(ks, p):
    """The table over problem `p` (an address): [name, elem_bytes, count, offset, marks]."""
    ks.ks_debug_problem_array.restype = ctypes.c_uint32
    ks.ks_debug_problem_array.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    out, n = [], ks.ks_debug_problem_array(p, 0xFFFFFFFF, None, None, None, None, None)
    for i in range(n):
        name, eb, cnt, off, marks = ctypes.c_char_p(), ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        assert ks.ks_debug_problem_array(p, i, ctypes.byref(name), ctypes.byref(eb), ctypes.byref(cnt), ctypes.byref(off), ctypes.byref(marks)) == n
        out.append([name.value.decode(), int(eb.value), int(cnt.value), int(off.value), int(marks.value)])
    return out


def solve_raw(ks, p):
    """ks_problem_upload + ks_solve_dev of the ks_problem at address `p` into arrays of this function's own: every result array the struct states a length for, as hex."""
    raw = ctypes.string_at(p, SIZEOF)
    P, T, K, R, NM = (_u32(raw, SCALARS[k]) for k in ("P", "T", "K", "R", "max_new_nodes"))
    TW = (T + 63) // 64
    sizes = {"pod_node": 4 * P, "pod_stage": 4 * P, "pod_seq": 4 * P, "pod_reason": 4 * P, "unscheduled": 4 * P, "node_tmpl": 4 * NM, "node_types": 8 * NM * TW,
             "node_requests": 8 * NM * R, "node_requests_present": 4 * NM, "node_present": 4 * NM, "node_complement": 4 * NM, "node_mask": 8 * NM * K, "node_gt": 4 * NM * K,
             "node_lt": 4 * NM * K, "node_it_state": 4 * NM}
    bufs = {k: ctypes.create_string_buffer(max(v, 8)) for k, v in sizes.items()}
    res = _Result()
    for k, b in bufs.items():
        setattr(res, k, ctypes.addressof(b))
    d = ctypes.c_void_p()
    ks.ks_problem_upload.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    ks.ks_solve_dev.argtypes = [ctypes.c_void_p, ctypes.POINTER(_Result), ctypes.c_void_p]
    ks.ks_problem_free.argtypes = [ctypes.c_void_p]
    ks.ks_last_error.restype = ctypes.c_char_p
    rc = ks.ks_problem_upload(p, 0, ctypes.byref(d))
    assert rc == 0, ks.ks_last_error()
    try:
        rc = ks.ks_solve_dev(d, ctypes.byref(res), None)
        assert rc == 0, ks.ks_last_error()
    finally:
        ks.ks_problem_free(d)
    N, U = int(res.n_new), int(res.n_unscheduled)
    used = {"pod_node": 4 * P, "pod_stage": 4 * P, "pod_seq": 4 * P, "pod_reason": 4 * P, "unscheduled": 4 * U, "node_tmpl": 4 * N, "node_types": 8 * N * TW,
            "node_requests": 8 * N * R, "node_requests_present": 4 * N, "node_present": 4 * N, "node_complement": 4 * N, "node_mask": 8 * N * K, "node_gt": 4 * N * K,
            "node_lt": 4 * N * K, "node_it_state": 4 * N}
    out = {k: bufs[k].raw[:used[k]].hex() for k in sizes}
    out["n_new"], out["n_unscheduled"], out["err"] = N, U, int(res.stats[7])
    return out


def rebuilt(ks, p, strip=(), exact=True):
    """(address of a copy of the ks_problem at `p` whose every array is an exact-length copy, the buffers that keep it alive).  `strip`: rows passed as NULL instead.
    exact=False: the handle's own arrays, only the stripped ones NULL."""
    raw = bytearray(ctypes.string_at(p, SIZEOF))
    keep = [raw]
    for name, eb, cnt, off, marks in rows_of(ks, p):
        ptr = int.from_bytes(raw[off:off + 8], "little")
        if name in strip or (exact and not (ptr and cnt)):
            new = 0
        elif not exact:
            new = ptr
        else:
            buf = ctypes.create_string_buffer(ctypes.string_at(ptr, cnt * eb), cnt * eb)      # exactly count * elem_bytes: no terminator, no slack
            keep.append(buf)
            new = ctypes.addressof(buf)
        raw[off:off + 8] = new.to_bytes(8, "little")
    struct = (ctypes.c_char * SIZEOF).from_buffer(raw)
    keep.append(struct)
    return ctypes.addressof(struct), keep


def _plain(r):
    return [r.canonical(), sorted(r.reasons.items())]


def examine(Sm, fp, flip=True, strip=()):
    """Everything the tests assert about one flat problem, from the handle `fp`."""
    ks, kh = Sm.libs()
    kh.ksh_problem.restype, kh.ksh_problem.argtypes = ctypes.c_void_p, [ctypes.c_void_p]
    p = kh.ksh_problem(fp._h)
    raw = ctypes.string_at(p, SIZEOF)
    rows = rows_of(ks, p)
    out = {"rows": rows, "scalars": {k: _u32(raw, o) for k, o in SCALARS.items()}, "oracle_like": _plain(fp.solve())}
    bare, keep0 = rebuilt(ks, p, strip, exact=False) if strip else (p, None)
    out["original"] = solve_raw(ks, bare)
    copy, keep = rebuilt(ks, p, strip)
    out["rebuilt"] = solve_raw(ks, copy)
    craw = ctypes.string_at(copy, SIZEOF)
    out["null"] = [name for name, eb, cnt, off, marks in rows if not int.from_bytes(craw[off:off + 8], "little")]      # what the rebuilt problem passes as NULL
    if flip:
        base, moved = fp.fingerprint(), {}
        for name, eb, cnt, off, marks in rows:
            ptr = int.from_bytes(raw[off:off + 8], "little")
            if not (ptr and cnt):
                continue
            at = ptr + cnt * eb - 1      # the LAST byte the table counts: inside the vector, and inside what the fingerprint hashes
            byte = ctypes.string_at(at, 1)
            ctypes.memmove(at, bytes([byte[0] ^ 0x40]), 1)
            moved[name] = fp.fingerprint() != base
            ctypes.memmove(at, byte, 1)
        assert fp.fingerprint() == base
        out["moved"] = moved
    return out


def device_run(Sm, job):
    if job["kind"] == "case":
        name, _, variant = job["name"].partition("/")
        fp = Sm.FlatProblem(build_case(name))
        try:
            return examine(Sm, fp, flip=not variant, strip=("it_price", "it_price_lo") if variant == "no_prices" else ())
        finally:
            fp.close()
    snap, pod_node, sets, _ = shared_snapshot()
    parsed = Sm.ParsedProblem(snap)
    flats = Sm.open_whatifs(parsed, pod_node, sets, derive=False)
    try:
        shared, _, _ = Sm.solve_batch(flats)      # (uploads each against the resident snapshot: ks_problem_upload_shared)
        return {"shared": [_plain(r) for r in shared], "each": [examine(Sm, f) for f in flats]}
    finally:
        for f in flats:
            f.close()
        parsed.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
jobs = json.loads(open(sys.argv[1]).read())
if jobs["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_problem_arrays as A
out = {}
for name, job in jobs["jobs"].items():
    try:
        out[name] = A.device_run(S, job)
    except Exception as e:
        import traceback
        out[name] = {"error": traceback.format_exc()[-1500:]}
print("RESULT " + json.dumps(out))
"""

JOBS = dict({v: {"kind": "case", "name": v} for v in VARIANTS}, shared={"kind": "shared"})
_RUNS, _ORACLE = {}, {}


def run(request, backend):
    """One child per backend for the whole module: every job in one fresh process (the pytest process keeps the product's libraries)."""
    if backend not in _RUNS:
        sim = backend == "emu" or bool(os.environ.get("KS_TEST_SIM"))
        tmp = request.getfixturevalue("tmp_path_factory").mktemp("problem_arrays")
        path = os.path.join(str(tmp), "jobs.json")
        with open(path, "w") as fh:
            json.dump({"sim": sim, "jobs": JOBS}, fh)
        env = dict(os.environ)
        env.pop("KS_TEST_SIM", None)
        pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=600)
        line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
        _RUNS[backend] = json.loads(line[-1][7:]) if line else {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in JOBS}
    return _RUNS[backend]


def oracle(name):
    from oracle import oracle_py as O
    if name not in _ORACLE:
        problems = shared_snapshot()[3] if name == "shared" else [build_case(name.partition("/")[0])]
        _ORACLE[name] = [json.loads(json.dumps(_plain(O.solve(pr)))) for pr in problems]
    return _ORACLE[name]


def examined(request, backend):
    """(label, what `examine` found) for every flat problem of the run: the variants and the two what-ifs over the shared snapshot."""
    res = run(request, backend)
    assert all("error" not in v for v in res.values()), {k: v["error"] for k, v in res.items() if "error" in v}
    return [(v, res[v]) for v in VARIANTS] + [(f"shared[{i}]", e) for i, e in enumerate(res["shared"]["each"])]


# ---------------------------------------------------------------------------------------------------------------- the tests
def test_the_rows_cover_every_pointer_of_the_struct(request):
    assert sorted(list(SCALARS.values()) + PADDING) == sorted(set(SCALARS.values()) | set(PADDING))
    for label, got in examined(request, "emu"):
        offs = [r[3] for r in got["rows"]]
        assert len(set(offs)) == len(offs) and all(o % 8 == 0 and o + 8 <= SIZEOF for o in offs), label
        covered = set()
        for o in offs:
            covered |= {o, o + 4}
        four = set(SCALARS.values()) | set(PADDING)
        assert not covered & four, label
        assert covered | four == set(range(0, SIZEOF, 4)), (label, sorted(set(range(0, SIZEOF, 4)) - covered - four))
        assert all(r[1] in (1, 2, 4, 8) for r in got["rows"]), label


def test_names_are_unique_and_one_row_is_not_fingerprinted(request):
    for label, got in examined(request, "emu"):
        names = [r[0] for r in got["rows"]]
        assert len(set(names)) == len(names), label
        assert [r[0] for r in got["rows"] if r[4] & NOT_FINGERPRINTED] == ["it_price_lo"], label
        assert [r[0] for r in got["rows"] if r[4] & NULLABLE] == ["it_price", "it_price_lo"], label
        assert {"tmpl.present", "en.mask", "cls.gt", "flt.it_state"} <= set(names), label      # a ks_reqsets member appears as its six arrays


def test_the_cases_reach_every_count_expression(request):
    by = dict(examined(request, "emu"))
    sc = {k: v["scalars"] for k, v in by.items()}
    cnt = {k: {r[0]: r[2] for r in v["rows"]} for k, v in by.items()}
    assert sc["r3"]["R"] == 3 and sc["r9"]["R"] == 9
    assert sc["ports"]["C"] > 0 and cnt["ports"]["ports"] > cnt["ports_no_pods"]["ports"] > 0      # existing reservations, then the classes' ports
    assert sc["ports_no_pods"]["P"] == 0 and sc["ports_no_pods"]["C"] == 0
    assert sc["volumes"]["ND"] == 1 and sc["volumes"]["SW"] == 1 and cnt["volumes"]["vol_list"] > 0 and cnt["volumes"]["en_vol_set"] > 0
    assert sc["filter"]["G"] >= 1 and sc["filter"]["flt.n"] > 0
    assert sc["anti"]["GH"] >= 1 and cnt["anti"]["grph_count"] > 0
    assert sc["it_in"]["S"] > 1 and sc["it_in"]["SC"] > 1 and cnt["it_in"]["hn_list"] > 0
    assert {"it_price", "it_price_lo"} <= set(by["r3/no_prices"]["null"]) and not {"it_price", "it_price_lo"} & set(by["r3"]["null"]) and cnt["r3/no_prices"]["it_price"] > 0
    assert all({r[0] for r in v["rows"] if not r[2]} <= set(v["null"]) for v in by.values())      # an array of no elements went in as NULL
    # together the cases give every row at least one element, so the byte flips below reach every array
    assert not [n for n in cnt["r3"] if not any(c[n] for c in cnt.values())]


def check_rebuilds(request, backend):
    """Every rebuild equals the original handle's arrays solved the same way, byte for byte, and the oracle.  The two what-ifs flattened over one snapshot go through
    ks_problem_upload_shared as a batch and, each by itself, through ks_problem_upload: the same results."""
    for label, got in examined(request, backend):
        assert got["original"]["err"] == 0 and got["rebuilt"] == got["original"], label
        assert got["original"]["pod_node"] or got["scalars"]["P"] == 0, label
    res = run(request, backend)
    for v in VARIANTS:
        assert res[v]["oracle_like"] == oracle(v)[0], v
    assert res["shared"]["shared"] == [e["oracle_like"] for e in res["shared"]["each"]] == oracle("shared")


def test_exact_length_rebuild_solves_to_the_same_bytes(request):
    check_rebuilds(request, "emu")


def test_a_flipped_byte_moves_the_fingerprint_unless_the_row_says_not(request):
    seen = set()
    for label, got in examined(request, "emu"):
        if "moved" not in got:
            continue
        marks = {r[0]: r[4] for r in got["rows"]}
        for name, moved in got["moved"].items():
            assert moved == (not marks[name] & NOT_FINGERPRINTED), (label, name)
            seen.add(name)
    assert seen == {r[0] for r in examined(request, "emu")[0][1]["rows"]}      # every row was flipped in some problem, it_price_lo among them


def c_program(tmp_path, libdir, case):
    """tests/cabi_usage_arrays.c as C99 with -Wall -Werror -pedantic against the libraries in `libdir`, over one case: its output."""
    exe = str(tmp_path / "cabi_usage_arrays")
    if not os.path.exists(exe):
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_arrays.c"),
                               "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    f = tmp_path / f"{case}.ksp"
    f.write_text(build_case(case).to_ksp())
    out = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_exact_length_rebuild_from_c_on_the_emulator(tmp_path):
    """The same rebuild from plain C with malloc'ed buffers (what the sanitizer builds run): every row walked, the copy uploaded and solved like the original."""
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    libdir = build_sim.build()
    for case in ("volumes", "it_in", "ports_no_pods"):
        out = c_program(tmp_path, libdir, case)
        assert "(1 not fingerprinted)" in out and "exact-length copy: the same result" in out, out
