"""What the C ABI's host half refuses BEFORE it touches a device, call by call: the return code and the exact words of ksh_last_error().  No GPU is needed and none
is used: every input here is one the library turns away in its argument checks, and no pointer is passed that a check does not look at first.  Driven through ctypes
on a CDLL object of its own (no argtypes shared with karpenter_core_amd.scheduler): a pointer is a c_void_p or None, a 64-bit integer is spelled out."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as ge
from karpenter_core_amd import fake, model as M, scheduler as S, workloads as W

INVALID, UNSUPPORTED = S.KS_ERR_INVALID, S.KS_ERR_UNSUPPORTED
NULL_ARG = (INVALID, "null argument")
NO_RESULT = (INVALID, "the handle holds no result: solve it first (or the last solve failed)")
KS_FLAG_STATS, BAD_FLAG = 2, 1 << 30
NN, NP, NT, WORDS = 2, 3, 2, 1      # the snapshot below: 2 nodes, 3 bound pods, 2 instance types (one 64-bit word of type bits)


_ALIVE = []      # every array a pointer was taken of stays alive for the whole run: no call here ever sees freed memory


def ptr(a):
    _ALIVE.append(a)
    return ctypes.c_void_p(a.ctypes.data)


def u32(*xs):
    return np.asarray(xs, dtype=np.uint32)


def u64(n):
    return np.zeros(n, dtype=np.uint64)


@pytest.fixture(scope="module")
def kh():
    ge.build()
    lib = ctypes.CDLL(S.libs()[1]._name)
    lib.ksh_last_error.restype = ctypes.c_char_p

    def call(name, *args):
        rc = getattr(lib, name)(*args)
        return rc, (lib.ksh_last_error().decode() if rc != S.KS_OK else "")
    lib.call = call
    return lib


@pytest.fixture(scope="module")
def world(kh):
    """The snapshot (2 nodes of 2 instance types, 3 bound pods), parsed; a second parse of it for the calls that change it; a handle that was opened over it and never
    uploaded or solved."""
    its, _, nodes, _ = W.cluster_snapshot(existing=2, sizes=1, seed=3)
    names = []
    for n in nodes:
        if n.labels[fake.LABEL_INSTANCE_TYPE] not in names:
            names.append(n.labels[fake.LABEL_INSTANCE_TYPE])
    names += [t.name for t in its if t.name not in names]
    its = [t for t in its if t.name in names[:NT]]
    rs = np.random.RandomState(0)
    few = [[W.generic_pod(rs, "pod-a"), W.generic_pod(rs, "pod-b")], [W.generic_pod(rs, "pod-c")]]
    snap, pod_node = W.snapshot_problem(its, fake.provisioner("default", len(its)), nodes, few, False)
    assert (len(snap.nodes), len(snap.pods), len(snap.instance_types), len(snap.provisioners)) == (NN, NP, NT, 1)
    text = snap.to_ksp().encode()

    def parse():
        p = ctypes.c_void_p()
        assert kh.ksh_parse(text, ctypes.c_size_t(len(text)), ctypes.byref(p)) == S.KS_OK
        return p
    w = dict(snap=snap, text=text, pn=np.asarray(pod_node, dtype=np.int32), parsed=parse(), scratch=parse(), handle=ctypes.c_void_p())
    assert kh.ksh_open_parsed(w["parsed"], 0, ctypes.byref(w["handle"])) == S.KS_OK
    yield w
    kh.ksh_close(w["handle"])
    kh.ksh_parsed_free(w["parsed"])
    kh.ksh_parsed_free(w["scratch"])


def test_text_doors(kh, world):
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_parse", b"", ctypes.c_size_t(0), ctypes.byref(out)) == (INVALID, "KSP1: unexpected end of input") and out.value is None
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_open", b"", ctypes.c_size_t(0), 0, ctypes.byref(out)) == (INVALID, "KSP1: unexpected end of input") and out.value is None
    hs = (ctypes.c_void_p * 1)(1)
    assert kh.call("ksh_open_whatifs", b"", ctypes.c_size_t(0), 0, 1, ptr(u32(0, 1)), ptr(u32(0)), None, 1, hs) == (INVALID, "KSP1: unexpected end of input") and hs[0] is None
    # the snapshot as text: no bindings, a candidate that is no node
    t, n = world["text"], ctypes.c_size_t(len(world["text"]))
    hs = (ctypes.c_void_p * 1)(1)
    assert kh.call("ksh_open_whatifs", t, n, 0, 1, ptr(u32(0, 1)), ptr(u32(0)), None, 1, hs) == (INVALID, "no bindings (pod_node)") and hs[0] is None
    assert kh.call("ksh_open_whatifs", t, n, 0, 1, ptr(u32(0, 1)), ptr(u32(NN)), ptr(world["pn"]), 1, hs) == (INVALID, "candidate node out of range")


def test_handles_without_a_device_or_a_result(kh, world):
    h, out = world["handle"], ctypes.c_void_p(1)
    hv = (ctypes.c_void_p * 1)(h)
    assert kh.call("ksh_open_parsed", None, 0, ctypes.byref(out)) == NULL_ARG and out.value is None
    assert kh.call("ksh_open_parsed", world["parsed"], 0, None) == NULL_ARG
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_open_batch", None, None, 0, ctypes.byref(out)) == NULL_ARG and out.value is None
    assert kh.call("ksh_open_batch", world["parsed"], None, 0, ctypes.byref(out)) == NULL_ARG
    assert kh.call("ksh_solve_from_batch", None, None, 0, 0, None, None) == NULL_ARG
    assert kh.call("ksh_solve_from_batch", world["parsed"], None, 0, 0, None, None) == NULL_ARG
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_pods_ingest", None, 1, ctypes.byref(out), None) == NULL_ARG and out.value is None
    assert kh.call("ksh_pods_ingest", None, 0, None, None) == NULL_ARG
    assert kh.call("ksh_pods_count", None, None, None) == NULL_ARG
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_result_text", None, ctypes.byref(out)) == NULL_ARG and out.value is None
    assert kh.call("ksh_result_text", h, None) == NULL_ARG
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_result_text", h, ctypes.byref(out)) == NO_RESULT and out.value is None
    row = u64(2 + WORDS)
    assert kh.call("ksh_result_summary", None, ptr(row), WORDS) == NULL_ARG
    assert kh.call("ksh_result_summary", h, None, WORDS) == NULL_ARG
    assert kh.call("ksh_result_summary", h, ptr(row), WORDS) == NO_RESULT
    assert kh.call("ksh_result_summaries", hv, 1, ptr(row), WORDS) == NO_RESULT
    arrays = np.zeros(64, dtype=np.uint64)      # (room for a ksh_result_arrays)
    assert kh.call("ksh_result_arrays_get", None, ptr(arrays)) == NULL_ARG
    assert kh.call("ksh_result_arrays_get", h, None) == NULL_ARG
    assert kh.call("ksh_result_arrays_get", h, ptr(arrays)) == (INVALID, "result arrays before a solve")
    # opened, never uploaded or solved: everything that reads a result on the device
    node, ids, masks, counts = u32(0), u64(1), u64(WORDS), u32(0)
    assert kh.call("ksh_result_records_dev", hv, 1, ptr(ids), WORDS, None) == (INVALID, "records before solve")
    assert kh.call("ksh_price_filter", hv, 1, ptr(node), ptr(np.zeros(1)), None, ptr(masks), WORDS, ptr(counts)) == (INVALID, "price filter before solve")
    i32 = [np.zeros(1, dtype=np.int32) for _ in range(3)]
    assert kh.call("ksh_launch_pick", hv, 1, ptr(node), ptr(i32[0]), ptr(i32[1]), ptr(i32[2]), ptr(np.zeros(1))) == (INVALID, "launch pick before solve")
    assert kh.call("ksh_types_subset", hv, 1, ptr(node), ptr(masks), WORDS, ptr(counts)) == (INVALID, "subset test before solve")
    cmd_in = np.zeros(16, dtype=np.uint64)      # (room for a ks_command_inputs; not read before the refusal)
    rows = u64(256)
    for handles in (hv, (ctypes.c_void_p * 1)(None)):
        assert kh.call("ksh_command_rows", handles, 1, ptr(ids), ptr(cmd_in), WORDS, ptr(rows), None) == (INVALID, "command rows before solve")
        assert kh.call("ksh_replacement_rows", handles, 1, ptr(ids), ptr(u32(0)), WORDS, ptr(rows), ptr(rows), ctypes.c_uint64(0), ptr(u64(1)), None) == (INVALID, "replacement rows before solve")
    assert kh.call("ksh_command_rows", None, 1, ptr(ids), ptr(cmd_in), WORDS, ptr(rows), None) == NULL_ARG
    assert kh.call("ksh_replacement_rows", None, 1, ptr(ids), ptr(u32(0)), WORDS, ptr(rows), ptr(rows), ctypes.c_uint64(0), ptr(u64(1)), None) == NULL_ARG
    shard = u32(0, 1)
    assert kh.call("ksh_solve_whatifs_sharded", None, ptr(shard), 1, ptr(ids), WORDS, ptr(rows), None) == NULL_ARG
    assert kh.call("ksh_solve_whatifs_sharded", hv, None, 1, ptr(ids), WORDS, ptr(rows), None) == NULL_ARG
    assert kh.call("ksh_solve_whatifs_sharded", hv, ptr(shard), 1, None, WORDS, ptr(rows), None) == NULL_ARG
    assert kh.call("ksh_solve_whatifs_sharded", hv, ptr(shard), 1, ptr(ids), WORDS, None, None) == NULL_ARG
    assert kh.call("ksh_solve_whatifs_sharded", hv, ptr(shard), 1, ptr(ids), WORDS, ptr(rows), None) == \
        (INVALID, "a what-if that is not resident (ksh_upload / ksh_upload_batch / ksh_open_whatifs_derived first)")
    for hh in (None, h):
        assert kh.call("ksh_debug_grid", hh, ptr(rows)) == (INVALID, "grid of a handle that was not uploaded")
        assert kh.call("ksh_debug_classes", hh, None, None) == (INVALID, "class tables of a handle that was not uploaded")
        for f in ("ksh_pack_width", "ksh_pack_lean", "ksh_pack_row", "ksh_rr_status"):      # (these four set no message)
            assert getattr(kh, f)(hh, ptr(np.zeros(2, dtype=np.int32))) == INVALID
    assert kh.call("ksh_debug_pod_classes", None, ptr(u32(0, 0, 0))) == NULL_ARG
    assert kh.call("ksh_debug_pod_classes", h, None) == NULL_ARG


def test_whatifs_over_the_snapshot(kh, world):
    P, pn, off, hs = world["parsed"], ptr(world["pn"]), ptr(u32(0, 1)), (ctypes.c_void_p * 1)(1)
    assert kh.call("ksh_open_whatifs_parsed", P, 0, 1, off, ptr(u32(NN)), pn, 1, hs) == (INVALID, "candidate node out of range") and hs[0] is None
    assert kh.call("ksh_open_whatifs_parsed", P, 0, 1, off, ptr(u32(0)), None, 1, hs) == (INVALID, "no bindings (pod_node)")
    hs[0] = 1
    assert kh.call("ksh_open_whatifs_derived", P, 0, 1, off, ptr(u32(NN)), pn, 0, hs) == (INVALID, "candidate node out of range") and hs[0] is None
    assert kh.call("ksh_open_whatifs_derived", P, KS_FLAG_STATS, 1, off, ptr(u32(0)), pn, 0, hs) == (UNSUPPORTED, "derived what-ifs carry no reference-algorithm statistics")
    assert kh.call("ksh_open_whatifs_derived", P, 0, 1, off, ptr(u32(0)), None, 0, hs) == (INVALID, "no bindings (pod_node)")
    assert kh.call("ksh_check_whatif_derivation", P, 0, ptr(u32(0)), 1, None) == (INVALID, "no bindings (pod_node)")
    out = ctypes.c_uint64(0)
    assert kh.call("ksh_snapshot_fingerprint", None, pn, 0, 0, ctypes.byref(out)) == NULL_ARG
    assert kh.call("ksh_snapshot_fingerprint", P, pn, 0, 0, None) == NULL_ARG
    for cold in (0, 1):
        assert kh.call("ksh_snapshot_fingerprint", P, None, 0, cold, ctypes.byref(out)) == (INVALID, "no bindings")
    n = ctypes.c_uint32()
    assert kh.call("ksh_snapshot_bindings", None, None, 0, ctypes.byref(n), ctypes.byref(n)) == NULL_ARG
    assert kh.call("ksh_snapshot_bindings", P, ptr(np.zeros(NP, dtype=np.int32)), NP, None, None) == (INVALID, "no ksh_env_apply yet: the caller holds the bindings")
    c = ctypes.c_int()
    assert kh.call("ksh_snapshot_it_state", None, 1, ctypes.byref(c), ctypes.byref(n)) == NULL_ARG
    assert kh.call("ksh_snapshot_it_state", P, 1, None, ctypes.byref(n)) == NULL_ARG
    assert kh.call("ksh_snapshot_it_state", P, 1, ctypes.byref(c), None) == NULL_ARG
    assert kh.call("ksh_snapshot_it_state", P, 1, ctypes.byref(c), ctypes.byref(n)) == (INVALID, "the snapshot was not flattened yet")
    # ... and flattened (the fingerprint does it), the states of the snapshot's lattice are numbered from 1
    assert kh.call("ksh_snapshot_fingerprint", P, pn, 0, 0, ctypes.byref(out)) == (S.KS_OK, "")
    assert kh.call("ksh_snapshot_it_state", P, 0, ctypes.byref(c), ctypes.byref(n)) == (INVALID, "instance-type state out of range")
    assert kh.call("ksh_snapshot_it_state", P, 1 << 20, ctypes.byref(c), ctypes.byref(n)) == (INVALID, "instance-type state out of range")


def block_struct(cls, b, **kw):
    """The ctypes mirror `cls` of a binary block, from the dict the model's writers make; `kw` overrides fields (a pointer as an int or None)."""
    v = dict(n_strings=b["n_strings"], n_words=b["n_words"], str_off=b["str_off"].ctypes.data, str_bytes=b["str_bytes"].ctypes.data, words=b["words"].ctypes.data,
             str_bytes_len=int(b["str_bytes"].size))
    for k in ("n_events", "n_pdbs"):
        if k in b:
            v[k] = b[k]
    v.update(kw)
    return cls(**v)


def string_table_cases(cls, b, what):
    """(block, refusal) for what every block's string table is refused for; `b` has at least two strings of different offsets."""
    so = b["str_off"]
    assert b["n_strings"] >= 2 and so[1] < so[2]
    swapped = so.copy(); swapped[1], swapped[2] = so[2], so[1]
    return [(block_struct(cls, b, str_off=None), NULL_ARG), (block_struct(cls, b, str_bytes=None), NULL_ARG),
            (block_struct(cls, b, str_off=swapped.ctypes.data), (INVALID, what + " block: string offsets not ascending")),
            (block_struct(cls, b, str_bytes_len=int(so[-1]) - 1), (INVALID, what + " block: string offsets reach beyond str_bytes_len"))], swapped


def test_env_block(kh, world):
    b = M.env_to_block(world["snap"])
    cases, keep = string_table_cases(S._EnvBlock, b, "env")
    cases.append((block_struct(S._EnvBlock, b, words=None), NULL_ARG))
    for blk, refusal in cases:
        out = ctypes.c_void_p(1)
        assert kh.call("ksh_env_ingest", ctypes.byref(blk), ctypes.byref(out), None) == refusal and out.value is None
    out = ctypes.c_void_p(1)
    assert kh.call("ksh_env_ingest", None, ctypes.byref(out), None) == NULL_ARG and out.value is None
    assert kh.call("ksh_env_ingest", ctypes.byref(block_struct(S._EnvBlock, b)), None, None) == NULL_ARG
    del keep


def test_env_apply_and_the_delta_block(kh, world):
    P, pn = world["scratch"], ptr(world["pn"])
    b = M.delta_to_block([("node-", "nobody"), ("unbind", "no-pod")])
    cases, keep = string_table_cases(S._DeltaBlock, b, "delta")
    cases.append((block_struct(S._DeltaBlock, b, words=None), NULL_ARG))
    for blk, refusal in cases:
        info = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
        assert kh.call("ksh_env_apply_block", P, pn, ctypes.byref(blk), 0, info) == refusal and list(info) == [0, 0, 0, 0]
    good = block_struct(S._DeltaBlock, b)
    info = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert kh.call("ksh_env_apply_block", None, pn, ctypes.byref(good), 0, info) == NULL_ARG and list(info) == [0, 0, 0, 0]
    assert kh.call("ksh_env_apply_block", P, pn, None, 0, info) == NULL_ARG
    for flags in (2, BAD_FLAG, 3):
        assert kh.call("ksh_env_apply_block", P, pn, ctypes.byref(good), flags, info) == (INVALID, "ksh_env_apply_block: unknown flag bit")
    # the order of the refusals: null arguments, then the flag word, then the string table
    bad_table = cases[2][0]
    assert kh.call("ksh_env_apply_block", P, pn, ctypes.byref(block_struct(S._DeltaBlock, b, str_off=None)), BAD_FLAG, info) == NULL_ARG
    assert kh.call("ksh_env_apply_block", P, pn, ctypes.byref(bad_table), BAD_FLAG, info) == (INVALID, "ksh_env_apply_block: unknown flag bit")
    text = M.delta_to_ksd([("node-", "nobody")]).encode()
    info = (ctypes.c_uint32 * 4)(9, 9, 9, 9)
    assert kh.call("ksh_env_apply", None, pn, text, ctypes.c_size_t(len(text)), info) == NULL_ARG and list(info) == [0, 0, 0, 0]
    assert kh.call("ksh_env_apply", P, pn, None, ctypes.c_size_t(0), info) == NULL_ARG
    needs = (INVALID, "the first ksh_env_apply needs the bindings (pod_node) of the snapshot's pods")
    assert kh.call("ksh_env_apply", P, None, text, ctypes.c_size_t(len(text)), info) == needs
    assert kh.call("ksh_env_apply_block", P, None, ctypes.byref(good), 0, info) == needs
    far = world["pn"].copy(); far[0] = NN
    assert kh.call("ksh_env_apply", P, ptr(far), text, ctypes.c_size_t(len(text)), info) == (INVALID, "pod_node out of range")
    # an event that names nothing: refused with its index, the bindings handed over all the same -- after which other bindings are refused
    nothing = (INVALID, "event 0: NODE-: no state node named nobody (the events before it were applied)")
    assert kh.call("ksh_env_apply", P, pn, text, ctypes.c_size_t(len(text)), info) == nothing and list(info) == [0, NN, NP, 0]
    assert kh.call("ksh_env_apply_block", P, None, ctypes.byref(good), 0, info) == nothing
    other = world["pn"].copy(); other[0] = 1 - other[0]
    assert kh.call("ksh_env_apply", P, ptr(other), text, ctypes.c_size_t(len(text)), info) == \
        (INVALID, "the bindings passed differ from the ones the library holds since the last ksh_env_apply (pass NULL)")
    del keep


def commands(kh, P, flags=0, n=1, off=(0, 1), cand=(0,), pn=None, deleting=(), words=WORDS, rows=True, n_deleting=None):
    d = u32(*deleting) if deleting else None
    return kh.call("ksh_consolidation_commands", P, flags, n, None if off is None else ptr(u32(*off)), None if cand is None else ptr(u32(*cand)), pn, None if d is None else ptr(d),
                   len(deleting) if n_deleting is None else n_deleting, 0, 0, ptr(u64(256)) if rows else None, words, None)


def replacements(kh, P, flags=0, n=1, off=(0, 1), cand=(0,), pn=None, deleting=(), words=WORDS, heads=True, nodes=True, cap=4, total=True, n_deleting=None):
    d = u32(*deleting) if deleting else None
    return kh.call("ksh_replacement_commands", P, flags, n, None if off is None else ptr(u32(*off)), None if cand is None else ptr(u32(*cand)), pn, None if d is None else ptr(d),
                   len(deleting) if n_deleting is None else n_deleting, 0, ptr(u64(256)) if heads else None, ptr(u64(256)) if nodes else None, ctypes.c_uint64(cap),
                   ptr(u64(1)) if total else None, words, None)


def validations(kh, P, flags=0, n=1, off=(0, 1), nodes=(0,), expect=(0,), options=None, why=(0, 0), node_flags=(0, 0), pn=None, deleting=(), words=WORDS, rows=True, n_deleting=None):
    d = u32(*deleting) if deleting else None
    return kh.call("ksh_validate_commands", P, flags, n, None if off is None else ptr(u32(*off)), None if nodes is None else ptr(u32(*nodes)), None if expect is None else ptr(u32(*expect)),
                   None if options is None else ptr(options), None if why is None else ptr(u32(*why)), None if node_flags is None else ptr(u32(*node_flags)), pn,
                   None if d is None else ptr(d), len(deleting) if n_deleting is None else n_deleting, 0, ptr(u64(256)) if rows else None, words, None)


@pytest.mark.parametrize("call,name,row", [(commands, "consolidation commands", "command"), (replacements, "replacement commands", "replacement"), (validations, "validate commands", "validation")])
def test_command_calls(kh, world, call, name, row):
    """The three calls that simulate candidate sets share their whole-call refusals; `name` and `row` word them."""
    P, pn = world["parsed"], ptr(world["pn"])
    assert call(kh, None, pn=pn) == NULL_ARG
    assert call(kh, P, pn=pn, off=None) == NULL_ARG
    assert call(kh, P, pn=pn, n_deleting=1) == NULL_ARG
    assert call(kh, P, pn=pn, flags=BAD_FLAG) == (INVALID, name + ": unknown flag bit")
    assert call(kh, P, pn=pn, flags=BAD_FLAG, n=0) == (INVALID, name + ": unknown flag bit")
    assert call(kh, P, pn=pn, words=0) == (INVALID, f"{row} row too short: 0 words for {NT} instance types")
    assert call(kh, P, pn=pn, n=2, off=(0, 2, 1), **({"expect": (0, 0)} if call is validations else {})) == (INVALID, "candidate offsets not ascending")
    assert call(kh, P, pn=pn, **{"nodes" if call is validations else "cand": None}) == NULL_ARG
    assert call(kh, P, pn=pn, **{"nodes" if call is validations else "cand": (NN,)}) == (INVALID, "candidate node out of range")
    assert call(kh, P, pn=pn, deleting=(NN,)) == (INVALID, "deleting node out of range")


def test_command_calls_own_refusals(kh, world):
    P, pn = world["parsed"], ptr(world["pn"])
    assert commands(kh, P, pn=pn, rows=False) == NULL_ARG
    assert replacements(kh, P, pn=pn, heads=False) == NULL_ARG
    assert replacements(kh, P, pn=pn, total=False) == NULL_ARG
    assert replacements(kh, P, pn=pn, nodes=False) == NULL_ARG
    assert validations(kh, P, pn=pn, rows=False) == NULL_ARG
    assert validations(kh, P, pn=pn, expect=None) == NULL_ARG
    assert validations(kh, P, pn=pn, why=None) == NULL_ARG
    assert validations(kh, P, pn=pn, node_flags=None) == NULL_ARG
    assert validations(kh, P, pn=pn, expect=(1,), options=None) == NULL_ARG
    beyond = u64(WORDS); beyond[0] = 1 << NT      # a replacement option that is no instance type of the catalogue
    assert validations(kh, P, pn=pn, expect=(1,), options=beyond) == (INVALID, "command 0: type index out of range")


def test_the_loops_over_the_command_calls(kh, world):
    P, pn = world["parsed"], ptr(world["pn"])
    row, vrow, one, both, state = u64(256), u64(256), u32(0), u32(0, 1), u32(0)
    for f, extra in (("ksh_first_n_node_option", (100,)), ("ksh_single_node_option", ())):
        assert kh.call(f, P, 0, ptr(both), 2, *extra, pn, None, 0, 0, None, WORDS, None) == NULL_ARG
        assert kh.call(f, P, 0, None, 2, *extra, pn, None, 0, 0, ptr(row), WORDS, None) == NULL_ARG
        assert kh.call(f, P, BAD_FLAG, ptr(both), 2, *extra, pn, None, 0, 0, ptr(row), WORDS, None) == (INVALID, "consolidation commands: unknown flag bit")
        assert kh.call(f, P, 0, ptr(both), 2, *extra, pn, None, 0, 0, ptr(row), 0, None) == (INVALID, f"command row too short: 0 words for {NT} instance types")
        assert kh.call(f, P, 0, ptr(u32(0, NN)), 2, *extra, pn, None, 0, 0, ptr(row), WORDS, None) == (INVALID, "candidate node out of range")
        assert kh.call(f, P, 0, ptr(both), 2, *extra, pn, ptr(u32(NN)), 1, 0, ptr(row), WORDS, None) == (INVALID, "deleting node out of range")
    resume = lambda flags=0, cands=ptr(one), r=ptr(row), v=ptr(vrow), s=ptr(state): kh.call(      # noqa: E731
        "ksh_single_node_resume", P, flags, cands, 1, 0, ptr(both), ptr(both), pn, None, 0, 0, r, v, s, WORDS, None)
    assert resume(r=None) == NULL_ARG and resume(v=None) == NULL_ARG and resume(s=None) == NULL_ARG and resume(cands=None) == NULL_ARG
    assert resume(flags=BAD_FLAG) == (INVALID, "consolidation commands: unknown flag bit")
    assert resume(cands=ptr(u32(NN))) == (INVALID, "candidate node out of range")
    head, nodes, total, pos = u64(16), u64(256), u64(1), np.zeros(1, dtype=np.int32)
    option = lambda p=P, cands=ptr(one), why=ptr(both), deleting=None, nd=0, h=ptr(head), t=ptr(total), at=ptr(pos): kh.call(      # noqa: E731
        "ksh_replacement_option", p, 0, cands, 1, why, pn, deleting, nd, 0, h, ptr(nodes), ctypes.c_uint64(4), t, at, WORDS, None)
    for kw in (dict(p=None), dict(cands=None), dict(why=None), dict(nd=1), dict(h=None), dict(t=None), dict(at=None)):
        assert option(**kw) == NULL_ARG, kw
    assert option(cands=ptr(u32(NN))) == (INVALID, "candidate node out of range")
    assert option(deleting=ptr(u32(NN)), nd=1) == (INVALID, "deleting node out of range")
    retry = u32(7)
    assert kh.call("ksh_validate_empty_nodes", ptr(one), 1, ptr(both), ptr(both), ptr(both), None) == NULL_ARG
    for k in range(4):
        args = [ptr(one), ptr(both), ptr(both), ptr(both)]; args[k] = None
        assert kh.call("ksh_validate_empty_nodes", args[0], 1, args[1], args[2], args[3], ptr(retry)) == NULL_ARG
    action, out_nodes, out_n = u32(0), u32(0), u32(0)
    assert kh.call("ksh_emptiness_command", ptr(one), 1, ptr(both), None, ptr(out_nodes), ptr(out_n)) == NULL_ARG
    assert kh.call("ksh_emptiness_command", ptr(one), 1, ptr(both), ptr(action), ptr(out_nodes), None) == NULL_ARG
    assert kh.call("ksh_emptiness_command", None, 1, ptr(both), ptr(action), ptr(out_nodes), ptr(out_n)) == NULL_ARG
    assert kh.call("ksh_emptiness_command", ptr(one), 1, None, ptr(action), ptr(out_nodes), ptr(out_n)) == NULL_ARG
    assert kh.call("ksh_emptiness_command", ptr(one), 1, ptr(both), ptr(action), None, ptr(out_n)) == NULL_ARG


class CandidateArgs:
    """Valid inputs of ksh_consolidation_candidates / ksh_deprovisioning_candidates for the snapshot; a test spoils one thing at a time."""

    def __init__(self):
        self.node_flags, self.age = u32(0, 0), np.ones(NN)
        self.pod_flags, self.cost, self.prio = u32(0, 0, 0), np.zeros(NP), np.zeros(NP, dtype=np.int32)
        self.enabled, self.ttl, self.ttl_empty = u32(1), np.full(1, -1, dtype=np.int64), np.full(1, -1, dtype=np.int64)
        self.created, self.emptied = np.zeros(NN, dtype=np.int64), np.zeros(NN, dtype=np.int64)
        self.outs = [u32(0, 0), u32(0, 0), u32(0, 0), np.zeros(NN, dtype=np.int32), u32(0, 0), np.zeros(NN)]
        self.sizes = (NN, NP, 1)

    def inputs(self):
        return S._CandidateInputs(*self.sizes, 0, *[None if a is None else a.ctypes.data for a in (self.node_flags, self.age, self.pod_flags, self.cost, self.prio, self.enabled, self.ttl)])

    def out(self):
        return S._CandidatesOut(0, 0, *[None if a is None else a.ctypes.data for a in self.outs])

    def consolidation(self, kh, P, pn, deleting=None, n_deleting=0, pdbs=None):
        i, o = self.inputs(), self.out()
        return kh.call("ksh_consolidation_candidates", P, pn, deleting, n_deleting, ctypes.byref(i), None if pdbs is None else ctypes.byref(pdbs), 0, ctypes.byref(o), None)

    def deprovisioning(self, kh, P, pn, method=1, deleting=None, n_deleting=0, pdbs=None):
        i = S._DeprovisioningInputs(self.inputs(), 0, *[None if a is None else a.ctypes.data for a in (self.created, self.emptied, self.ttl_empty)], 0, 0)
        o = S._DeprovisioningOut(self.out(), 0, 0)
        return kh.call("ksh_deprovisioning_candidates", P, method, pn, deleting, n_deleting, ctypes.byref(i), None if pdbs is None else ctypes.byref(pdbs), 0, ctypes.byref(o), None)


def test_candidate_calls(kh, world):
    P, pn = world["parsed"], ptr(world["pn"])
    for what, run in (("consolidation candidates", CandidateArgs.consolidation), ("deprovisioning candidates", CandidateArgs.deprovisioning)):
        def spoiled(**kw):
            a = CandidateArgs()
            for k, v in kw.items():
                setattr(a, k, v)
            return a
        A = CandidateArgs()
        assert run(A, kh, None, pn) == NULL_ARG
        assert run(A, kh, P, pn, n_deleting=1) == NULL_ARG
        assert run(A, kh, P, None) == (INVALID, "no bindings (pod_node)")
        assert run(spoiled(sizes=(NN + 1, NP, 1)), kh, P, pn) == (INVALID, f"{what}: the input arrays are for {NN + 1} nodes / {NP} pods / 1 provisioners, the snapshot has {NN} / {NP} / 1")
        for field in ("node_flags", "age", "pod_flags", "cost", "prio", "ttl"):
            assert run(spoiled(**{field: None}), kh, P, pn) == NULL_ARG, field
        for k in range(6):
            a = CandidateArgs(); a.outs[k] = None
            assert run(a, kh, P, pn) == NULL_ARG, k
        assert run(A, kh, P, pn, deleting=ptr(u32(NN)), n_deleting=1) == (INVALID, "deleting node out of range")
        for bad in (NN, -2):
            far = world["pn"].copy(); far[2] = bad
            assert run(A, kh, P, ptr(far)) == (INVALID, "pod_node out of range")
        assert run(spoiled(node_flags=u32(0, 1 << 8)), kh, P, pn) == (INVALID, f"{what}: node 1: unknown flag bit")
        assert run(spoiled(node_flags=u32(4, 0)), kh, P, pn) == (INVALID, f"{what}: node 0: unknown flag bit")      # "true" without the annotation
        assert run(spoiled(age=np.asarray([1.0, np.inf])), kh, P, pn) == (INVALID, f"{what}: node 1: age is not finite")
        assert run(spoiled(pod_flags=u32(0, 0, 8)), kh, P, pn) == (INVALID, f"{what}: pod 2: unknown flag bit")
        assert run(spoiled(pod_flags=u32(0, 2, 0), cost=np.asarray([0.0, np.nan, 0.0])), kh, P, pn) == \
            (INVALID, f"{what}: pod 1: deletion cost is not finite")
        for ttl in (0, -2):
            assert run(spoiled(ttl=np.full(1, ttl, dtype=np.int64)), kh, P, pn) == \
                (INVALID, f"{what}: provisioner default: ttlSecondsUntilExpired {ttl} (the reference divides by a ttl of 0; -1 means none)")
        # the PDB block is read first, completely
        b = M.pdbs_to_block([M.PodDisruptionBudget(namespace="default", selector=M.LabelSelector({"my-label": "a"}), disruptions_allowed=1)])
        cases, keep = string_table_cases(S._PdbBlock, b, "pdb")
        cases.append((block_struct(S._PdbBlock, b, words=None), NULL_ARG))
        for blk, refusal in cases:
            assert run(A, kh, P, None, pdbs=blk) == refusal
        del keep
    assert CandidateArgs().deprovisioning(kh, P, pn, method=9) == (INVALID, "deprovisioning candidates: unknown method 9")
    assert CandidateArgs().deprovisioning(kh, P, pn, method=0) == (INVALID, "deprovisioning candidates: unknown method 0")
    a = CandidateArgs(); a.enabled = None
    assert a.consolidation(kh, P, pn) == NULL_ARG
    for field in ("created", "emptied", "ttl_empty"):
        a = CandidateArgs(); setattr(a, field, None)
        assert a.deprovisioning(kh, P, pn) == NULL_ARG, field
    a = CandidateArgs(); a.node_flags = u32(32, 0)
    assert a.deprovisioning(kh, P, pn) == (INVALID, "deprovisioning candidates: node 0: KSH_CAND_NODE_EMPTINESS_UNPARSABLE without KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP")
    a = CandidateArgs(); a.ttl_empty = np.full(1, -2, dtype=np.int64)
    assert a.deprovisioning(kh, P, pn) == (INVALID, "deprovisioning candidates: provisioner default: ttlSecondsAfterEmpty -2 (-1 means none)")
    assert kh.call("ksh_deprovisioning_candidates", P, 1, pn, None, 0, None, None, 0, None, None) == NULL_ARG
