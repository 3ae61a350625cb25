"""What the tests of the audit's six passes share (tests/audit_*_cases.py, tests/test_audit*.py): one descriptor per pass -- the binding's method and batch function,
the literal reference, the bit tables, the names of `checked` and of the counters -- and, over the descriptor, the comparison of the device pass with its reference, the
bodies the GPU tests have in common, the emulator's subprocess runner and the compile-and-run of the C usage programs.  Every function that audits takes the scheduler
module `S` it is to go through (the HIP libraries' or the emulator's).  The problems, tamper lists, shapes and verdicts are each pass's own, in its cases module."""
import copy
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import audit_firstfit_ref as FR
import audit_hostfit_ref as HR
import audit_limits_ref as LR
import audit_ref as A
import audit_spread_ref as SR
import audit_topo_ref as TR

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_PLACED = (("n_new", "n_new"), ("n_placed", "n_placed"))      # in every later pass's summary


def commit_numbers(S, flat, prob):
    """The commit numbers of the result on the device by the problem's OWN pod indices, through `ksh_placement_rows`: row k is the pod at position k of the problem's
    queue.  (`FlatProblem.pod_seq` goes by the pod the row names, which for a what-if over a snapshot is the snapshot's.)"""
    heads, rows, _ = S.placement_rows([flat], [0])
    seq = np.full(prob["P"], -1, dtype=np.int32)
    if rows is not None and prob["P"]:
        seq[prob["queue"][rows[:, S.KS_PLC_POSITION].astype(np.int64)]] = (rows[:, S.KS_PLC_STAGE_SEQ] >> np.uint64(32)).astype(np.uint32).view(np.int32)
    return seq


def _claimable(res):
    return copy.deepcopy({k: v for k, v in res.items() if k != "key_value"})


def flagged(flags):
    return {int(i): int(flags[i]) for i in np.nonzero(flags)[0]}


def _limits_extra(dev, ref):
    if dev["limited_templates"]:      # (with no limited template the pass examines no pod and skips none)
        assert dev["checked"]["PODS"] + dev["skipped_pods"] == len(ref["pod_flags"])


class Pass:
    """One pass of the audit as its tests see it.  method / batch: `FlatProblem.<method>`, `scheduler.<batch>`;  stem: the C names (ksh_<stem>, ks_<stem>_dev);  out: the
    binding's struct;  ref: the reference module, whose audit() returns `ref_returns` (None: a dict already);  gives: what compare() returns beside the device pass (None:
    the reference's dict);  counters: the scalars device and reference must agree on;  summary: (name, key or keys) of what summary() reports beside the bits and `checked`;
    pods_identity: every pod is examined or skipped;  extra: what fits no column, a function of (device pass, reference)."""

    def __init__(self, name, ref, pod_bits, node_bits=None, checked=None, ref_returns=None, gives=("pod_flags",), counters=(), summary=(), pods_identity=False, extra=None):
        self.name, self.ref, self.pod_bits, self.node_bits, self.checked, self.ref_returns, self.gives = name, ref, pod_bits, node_bits, checked, ref_returns, gives
        self.counters, self.summary_of, self.pods_identity, self.extra = counters, summary, pods_identity, extra
        self.seq = name != "audit"      # the first pass takes no commit numbers
        self.method = self.stem = "audit_" + name if self.seq else "audit"
        self.batch = self.method + "_batch"
        self.out = {"audit": "_AuditOut", "topology": "_AuditTopologyOut", "spread": "_AuditSpreadOut", "firstfit": "_AuditFirstFitOut", "limits": "_AuditLimitsOut",
                    "hostfit": "_AuditHostFitOut"}[name]
        self.tables = ("pod", "node") if node_bits else ("pod",)

    def run(self, flat, claimed=None, pod_seq=None):
        return getattr(flat, self.method)(claimed, pod_seq) if self.seq else flat.audit(claimed)

    def compare(self, S, flat, claimed=None, pod_seq=None):
        """The device pass and the reference's findings (`gives`) of the result `flat` holds -- or of `claimed` with `pod_seq` --, after asserting that device and reference
        agree bit for bit, `checked` and every counter included, and that the device's totals are the totals of its own flags."""
        dev = self.run(flat, claimed, pod_seq)
        res = flat.result_arrays() if claimed is None else claimed
        prob = self.ref.problem_arrays(S, flat)
        ref = self.ref.audit(prob, res, commit_numbers(S, flat, prob) if pod_seq is None else pod_seq) if self.seq else self.ref.audit(prob, res)
        if self.ref_returns:
            ref = dict(zip(self.ref_returns, ref))
        for t, bits in zip(self.tables, (self.pod_bits, self.node_bits)):
            d, r = dev[t + "_flags"], ref[t + "_flags"]
            assert d.shape == r.shape, (t, d.shape, r.shape)
            bad = np.nonzero(d != r)[0]
            assert not len(bad), (t, bad[:8], d[bad][:8], r[bad][:8])
            assert dev["n_%ss_flagged" % t] == int((r != 0).sum())
            assert dev[t + "_bit_count"] == {k: int(((r & v) != 0).sum()) for k, v in bits.items()}
        if self.checked:
            assert dev["checked"] == dict(zip(self.checked, ref["checked"])), (dev["checked"], ref["checked"])
        for k in self.counters:
            assert dev[k] == ref[k], (k, dev[k], ref[k])
        if self.pods_identity:
            assert dev["checked"]["PODS"] + dev["skipped_pods"] == len(ref["pod_flags"])
        if self.extra:
            self.extra(dev, ref)
        return (dev,) + tuple(ref[k] for k in self.gives) if self.gives else (dev, ref)

    def assert_clean(self, S, flat):
        dev = self.compare(S, flat)[0]
        for t in self.tables:
            assert not dev[t + "_flags"].any() and dev["n_%ss_flagged" % t] == 0, (t, dev[t + "_bit_count"])
        return dev

    def summary(self, dev):
        out = {t + "s": {k: v for k, v in dev[t + "_bit_count"].items() if v} for t in self.tables}
        if self.checked:
            out["checked"] = [dev["checked"][k] for k in self.checked]
        out.update((name, dev[k] if isinstance(k, str) else [dev[x] for x in k]) for name, k in self.summary_of)
        return out

    def same_runs(self, runs):
        return all(all(np.array_equal(r[t + "_flags"], runs[0][t + "_flags"]) for t in self.tables) and self.summary(r) == self.summary(runs[0]) for r in runs)


_LIMITS_COUNTERS = ("limited_templates", "skipped_nodes", "skipped_pods", "exact_nodes", "binding_nodes", "n_new", "n_placed")
PASSES = {p.name: p for p in (
    Pass("audit", A, A.POD, A.NODE, ref_returns=("pod_flags", "node_flags"), gives=("pod_flags", "node_flags"), summary=(("n_new", "n_new"), ("n_unscheduled", "n_unscheduled"))),
    Pass("topology", TR, TR.BITS, checked=TR.RULES, ref_returns=("pod_flags", "checked", "skipped_groups"), gives=("pod_flags", "checked"), counters=("skipped_groups",),
         summary=(("skipped", "skipped_groups"),) + _PLACED),
    Pass("spread", SR, SR.BITS, checked=SR.RULES, ref_returns=("pod_flags", "checked", "exact_pairs", "skipped_groups"), counters=("exact_pairs", "skipped_groups"),
         summary=(("exact", "exact_pairs"), ("skipped", "skipped_groups")) + _PLACED),
    Pass("firstfit", FR, FR.BITS, checked=FR.CHECKED, ref_returns=("pod_flags", "checked", "admitting_pairs", "skipped_pods"), counters=("admitting_pairs", "skipped_pods"),
         summary=(("admitting", "admitting_pairs"), ("skipped", "skipped_pods")) + _PLACED, pods_identity=True),
    Pass("limits", LR, LR.POD_BITS, LR.NODE_BITS, checked=LR.CHECKED, gives=None, counters=_LIMITS_COUNTERS, summary=tuple(zip(_LIMITS_COUNTERS, _LIMITS_COUNTERS)), extra=_limits_extra),
    Pass("hostfit", HR, HR.BITS, checked=HR.CHECKED, ref_returns=("pod_flags", "checked", "admitting_pairs", "skipped_pods", "eligible_groups", "skipped_groups"),
         counters=("admitting_pairs", "skipped_pods", "eligible_groups", "skipped_groups"), pods_identity=True,
         summary=(("admitting", "admitting_pairs"), ("skipped", "skipped_pods"), ("groups", ("eligible_groups", "skipped_groups"))) + _PLACED),
)}


# ---------------------------------------------------------------------------------------------------------------- the bodies the GPU tests share
WHATIF_SETS = [[0, 3], [5], [1, 2, 9], [7, 11], [4, 6, 8, 10, 12], [15]]


def refusals(D, S, problem, totals=None):
    """What every pass refuses, and the totals alone with no table given; `totals(out, flat)`: what the pass's own counters must say then."""
    ks, kh = S.libs()
    Out = getattr(S, D.out)
    resident, claimed_fn = getattr(kh, "ksh_" + D.stem), getattr(kh, "ksh_" + D.stem + "_claimed")
    f = S.FlatProblem(problem)
    f.upload(0)
    with pytest.raises(S.KSolveError) as e:      # nothing solved
        D.run(f)
    assert e.value.code == S.KS_ERR_INVALID
    f.solve(decode=False)
    resident.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_double)]
    hs = (ctypes.c_void_p * 1)(f._h)
    out = (Out * 1)()
    out[0].cap_pods, out[0].pod_flags = 64, None      # a table promised and not given
    assert resident(hs, 1, out, None) == S.KS_ERR_INVALID
    if D.node_bits:
        out[0].cap_pods, out[0].cap_nodes, out[0].node_flags = 0, 64, None
        assert resident(hs, 1, out, None) == S.KS_ERR_INVALID
    assert resident(hs, 1, None, None) == S.KS_ERR_INVALID
    assert resident(None, 1, out, None) == S.KS_ERR_INVALID
    out[0].cap_pods = 0      # the totals alone: no table needed
    if D.node_bits:
        out[0].cap_nodes = 0
    truncated = S.KSH_AUDIT_TRUNCATED_PODS | (S.KSH_AUDIT_TRUNCATED_NODES if D.node_bits else 0)
    assert resident(hs, 1, out, None) == S.KS_OK and out[0].n_pods == f.dims["P"] and out[0].truncated == truncated
    assert not D.seq or out[0].checked[0] == f.dims["P"]
    assert totals is None or totals(out[0], f)
    one_dev = getattr(ks, "ks_%s_dev" % D.stem)
    one_dev.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert one_dev(None, None, None) == S.KS_ERR_INVALID
    if D.seq:
        batch_dev = getattr(ks, "ks_%s_batch_dev" % D.stem)
        batch_dev.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        assert batch_dev(None, 1, None) == S.KS_ERR_INVALID
    res = f.result_arrays()
    seq = [f.pod_seq()] if D.seq else []
    many = dict(res, n_new=f.dims["P"] + 1)      # more new nodes than max_new_nodes
    with pytest.raises(S.KSolveError) as e:
        D.run(f, many, *seq)
    assert e.value.code == S.KS_ERR_INVALID
    if D.seq:
        with pytest.raises(S.KSolveError) as e:      # no commit numbers
            D.run(f, res)
        assert e.value.code == S.KS_ERR_INVALID
    claimed_fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_void_p] * len(seq) + [ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_double)]
    seq = [s.ctypes.data for s in seq]
    assert claimed_fn(f._h, None, *seq, out, None) == S.KS_ERR_INVALID
    ra = S._ResultArrays()      # the right dimensions and no arrays
    ra.n_pods, ra.n_existing, ra.types_words, ra.n_resources, ra.n_keys = f.dims["P"], f.dims["E"], (f.dims["T"] + 63) // 64, f.dims["R"], f.dims["K"]
    assert claimed_fn(f._h, ctypes.byref(ra), *seq, out, None) == S.KS_ERR_INVALID
    f.close()


def same_flags_every_run(D, S, problem, claim=None):
    """Three runs of the pass over `problem`'s result -- or over what `claim(flat)` makes of it, (claimed, pod_seq) -- raise the same flags and count the same; returns the first."""
    f = S.FlatProblem(problem)
    f.solve(decode=False)
    args = claim(f) if claim else ()
    runs = [D.run(f, *args) for _ in range(3)]
    assert D.same_runs(runs), [D.summary(r) for r in runs]
    f.close()
    return runs[0]


def derived_whatifs_are_clean(D, S, same, examined, after=None):
    """The decorated snapshot of tests/test_whatif_derived.py (spread, affinity, required anti-affinity over the hostname and the zone): the what-ifs flattened one by one
    are clean by the reference and by the device; the batch form says what one call each said; the device pass over the batch derived on the device -- one launch sequence
    over the results where they lie -- finds nothing either, `same(d)` being what a derived what-if and its flattened twin must agree on and `examined(d)` what must not be
    zero over the batch."""
    import test_whatif_derived as WD
    its, prov, nodes, bound, snap, pod_node = WD._topology_snapshot(24, 5, 11, spare=2, extras=False, anti=True)
    parsed = S.ParsedProblem(snap)
    flats = S.open_whatifs(parsed, pod_node, WHATIF_SETS, derive=False)
    S.solve_batch(flats, decode=False)
    plain = [D.assert_clean(S, f) for f in flats]
    batch = getattr(S, D.batch)(flats)      # the batch form over flattened problems says what one call each said
    for b, p in zip(batch, plain):
        assert np.array_equal(b["pod_flags"], p["pod_flags"]) and D.summary(b) == D.summary(p)
    derived = S.open_whatifs(parsed, pod_node, WHATIF_SETS, derive=True)
    S.solve_batch_resident(derived)
    got = getattr(S, D.batch)(derived)
    assert len(got) == len(WHATIF_SETS)
    for d, p in zip(got, plain):
        print(D.summary(d), D.summary(p))
        assert not d["pod_flags"].any() and d["n_pods_flagged"] == 0
        assert len(d["pod_flags"]) == len(p["pod_flags"]) and same(d) == same(p)
    assert sum(examined(d) for d in got) > 0 and sum(examined(p) for p in plain) > 0
    if after:
        after(derived, got)
    with pytest.raises(S.KSolveError) as e:      # a claimed result on a derived view
        D.run(derived[0], flats[0].result_arrays(), np.zeros(len(plain[0]["pod_flags"]), dtype=np.int32))
    assert e.value.code == S.KS_ERR_UNSUPPORTED
    for f in flats + derived:
        f.close()


# ---------------------------------------------------------------------------------------------------------------- the emulator in a subprocess; the C programs
def gate_names():
    """The names under which the emulator gates of the third, fourth and sixth pass report: (the what-ifs, every flattened problem, the what-ifs derived on the device)."""
    import test_rr_emulated as E
    whatifs = ["whatifs/%d" % i for i in range(4)] + ["wide_whatifs/%d" % i for i in range(len(E.WIDE_SETS))] + ["topology_whatifs/%d" % i for i in range(len(WHATIF_SETS))]
    flat = ["rr/" + c[0] for c in E.CASES] + ["no_rr/" + c[0] for c in E.CASES] + ["pack/" + c[0] for c in E.PACK_CASES] + whatifs
    derived = ["wide_whatifs_derived/%d" % i for i in range(len(E.WIDE_SETS))] + ["topology_whatifs_derived/%d" % i for i in range(len(WHATIF_SETS))]
    return whatifs, flat, derived


def run_emulated(child, *args):
    """Run `child` (its %(root)r and %(tests)r filled in) with `args`, JSON each, in a process of its own -- the emulator build replaces the two libraries for the whole
    process (tests/simlib.py) -- and return what its RESULT line holds."""
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None); env.pop("KS_NO_RR", None)
    env["KS_SIM_ALARM"] = "600"
    pr = subprocess.run([sys.executable, "-c", child % {"root": ROOT, "tests": HERE}] + [json.dumps(a) for a in args], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, pr.stdout[-2000:] + pr.stderr[-2000:]
    return json.loads(line[-1][7:])


def sim_libdir():
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    return build_sim.build()


def hip_libdir():
    import __graft_entry__ as ge
    ge.build()
    return os.path.join(ROOT, "karpenter_core_amd")


def run_c_program(tmp_path, libdir, name, problem, *args):
    """tests/<name>.c as C99 with -Wall -Werror -pedantic against the two libraries in `libdir`, run over `problem` with `args`; returns what it printed."""
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", name + ".c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    f = tmp_path / "problem.ksp"
    f.write_text(problem.to_ksp())
    out = subprocess.run([exe, str(f)] + list(args), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout
