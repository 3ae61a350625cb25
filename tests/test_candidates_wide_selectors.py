"""The wide-selector route of the two candidate calls (include/kshost.h KSH_CAND_WIDE_SELECTORS through ksh_consolidation_candidates_ex / ksh_deprovisioning_candidates_ex;
include/ksolve.h ks_selector_lists; kernel ks_cand_pods_lists in csrc/ksolve.hip) against the literal restatements in tests/candidates_ref.py and
tests/deprovisioning_ref.py.  As in tests/test_consolidation_candidates.py -- whose world builders are imported, not copied -- every world runs twice: unmarked on the
emulator build of the kernels in ONE child process, and marked `gpu` on the device in one more; every comparison happens here.  Costs are compared BITWISE.

Shapes are the smallest at which this kernel can go wrong: value sets around the old 62-value mask and the bisection's ends (1, 2, 63, 64, 65, 300) with the pod's value
first, last, in the middle, outside or absent; 40 keys with pods that carry none, one, ten or all of them; 300 one-per-application PDBs; 1, 2 and 65 namespaces whose
PDB indices interleave; listed-pod counts around the 256-lane block (255, 256, 257) with the only blocked pod last."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from karpenter_core_amd.model import Pod

import candidates_ref as R
import deprovisioning_ref as D
import test_consolidation_candidates as TCC
import test_deprovisioning_candidates as TDC
from test_consolidation_candidates import WORLDS, World, bits, node, pdb, pod, reference, sel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POISON32 = TCC.POISON32
provs = TCC.provs


# ---------------------------------------------------------------------------------------------------------------- worlds
SET_SIZES = [1, 2, 63, 64, 65, 300]


def w_sets():
    """One namespace per (operator, set size), its PDB `k <op> {v0 .. v(size-1)}`; six pods in each, one per node: the first member, the last, a middle one, a value
    other selectors mention but this one does not (v<size>; for 300 nobody mentions it), a value no selector mentions, and no `k` at all."""
    nodes, pods, pdbs = [], [], []
    for op in ("In", "NotIn"):
        for size in SET_SIZES:
            ns = f"{op.lower()}-{size}"
            pdbs.append(pdb(sel(exprs=[("k", op, [f"v{i}" for i in range(size)])]), ns=ns))
            for labels in ({"k": "v0"}, {"k": f"v{size - 1}"}, {"k": f"v{size // 2}"}, {"k": f"v{size}"}, {"k": "nobody-mentions-me"}, {"j": "v0"}):
                pods.append(pod(len(nodes), ns=ns, labels=labels))
                nodes.append(node())
    return World(nodes, pods, provs(), pdbs)


def w_keys():
    """40 mentioned keys k0 .. k39.  PDB 0: two requirements on one key (matchLabels k3=a plus k3 NotIn [b]) ; 1: an In list that repeats a value; 2: all 40 keys Exist;
    3: k39 In [z]; 4: k10 .. k19 absent and k20 present.  Pods, one per node: no label, only keys nobody mentions, exactly one key, ten keys, all 40."""
    pdbs = [pdb(sel({"k3": "a"}, [("k3", "NotIn", ["b"])])), pdb(sel(exprs=[("k5", "In", ["x", "y", "x"])])), pdb(sel(exprs=[(f"k{i}", "Exists", []) for i in range(40)])),
            pdb(sel(exprs=[("k39", "In", ["z"])])), pdb(sel(exprs=[(f"k{i}", "DoesNotExist", []) for i in range(10, 20)] + [("k20", "Exists", [])]))]
    every = {f"k{i}": "a" for i in range(40)}
    shapes = [{}, {"other": "1", "zz": "2"}, {"k39": "z"}, {"k39": "y", "zz": "2"}, {"k3": "a"}, {"k3": "b"}, {"k3": "a", "aa": "first-in-the-map"}, {"k5": "y"}, {"k5": "x", "k4": "q"}, {"k5": "z"},
              dict({f"k{i}": "q" for i in range(20, 30)}, unmentioned="u"), dict({f"k{i}": "q" for i in range(19, 29)}), dict(every), dict(every, k3="c"), dict(every, k3="b", k5="y"),
              dict(every, k3="c", k39="z"), {k: v for k, v in every.items() if k != "k17"}, dict({k: v for k, v in every.items() if k not in ("k3", "k17")}, k39="z")]
    return World([node() for _ in shapes], [pod(i, labels=l) for i, l in enumerate(shapes)], provs(), pdbs)


N_APPS = 300


def w_per_app():
    """300 PDBs app=a<i> and one pod per application on its own node: detail[i] is i.  Every third PDB allows a disruption and never blocks.  PDB 300 repeats 7's selector
    (7 wins), 301 repeats 5's (5 allows a disruption: 301 is the one that blocks).  302: app=a10 in namespace `other`, where a pod a10 and a pod a11 live.  303: a nil
    selector.  304: an empty selector in namespace `third`, which blocks whatever lives there."""
    pdbs = [pdb(sel({"app": f"a{i}"}), allowed=1 if i % 3 == 2 else 0) for i in range(N_APPS)]
    pdbs += [pdb(sel({"app": "a7"})), pdb(sel({"app": "a5"})), pdb(sel({"app": "a10"}), ns="other"), pdb(None), pdb(sel(), ns="third")]
    pods = [pod(i, labels={"app": f"a{i}", "pod-template-hash": f"h{i}"}) for i in range(N_APPS)]
    pods += [pod(N_APPS, ns="other", labels={"app": "a10"}), pod(N_APPS + 1, ns="other", labels={"app": "a11"}), pod(N_APPS + 2, ns="third", labels={"app": "a8"}), pod(N_APPS + 3, ns="third")]
    return World([node() for _ in range(N_APPS + 4)], pods, provs(), pdbs)


def w_namespaces(k):
    """k namespaces with pods, 3 k PDBs dealt round-robin, so a namespace's PDBs are k indices apart and every namespace's list interleaves with every other's.  Tier 0
    (indices < k) matches app=x but allows a disruption; tier 1 is app=x; tier 2 is app In [x, y]: a pod x must report its namespace's tier-1 index although tier 2
    matches too, a pod y the tier-2 index.  Namespace `lonely` has a PDB and no pod, `free` has pods and no PDB."""
    nss = [f"ns{i}" for i in range(k)]
    pdbs = []
    for b in range(3 * k):
        pdbs.append(pdb(sel({"app": "x"}) if b < 2 * k else sel(exprs=[("app", "In", ["y", "x"])]), ns=nss[(k - 1 - b) % k] if b >= 2 * k else nss[b % k], allowed=1 if b < k else 0))
    pdbs.insert(k, pdb(sel(), ns="lonely"))
    pods = []
    for ns in nss + ["free"]:
        for app in ("x", "y", "z"):
            pods.append(pod(len(pods), ns=ns, labels={"app": app}))
    return World([node() for _ in pods], pods, provs(), pdbs)


def w_pod_counts(n):
    """n listed pods, one per node, over two namespaces; only the LAST slot's pod is guarded."""
    pods = [pod(i, ns=f"ns{i % 2}", labels={"app": f"free{i % 5}"}) for i in range(n - 1)] + [pod(n - 1, ns="ns1", labels={"app": "guarded"})]
    return World([node() for _ in range(n)], pods, provs(), [pdb(sel({"app": "free1"}), ns="ns1", allowed=1), pdb(sel({"app": "guarded"}), ns="ns0"), pdb(sel({"app": "guarded"}), ns="ns1")])


def w_events_70():
    """80 one-per-application PDBs; a BIND through ksh_env_apply_block brings a pod whose app is the 70th value the selectors mention, then the call runs with pod_node = NULL."""
    new = Pod(uid="pod-2", namespace="default", labels={"app": "a69"})
    pdbs = [pdb(sel({"app": f"a{i}"}), allowed=1 if i < 10 else 0) for i in range(80)]
    w = World([node(), node()], [pod(0, labels={"app": "a0"}), pod(1, labels={"app": "nobody"})], provs(), pdbs, events=[("bind", "n1", new)])
    w.after = World([dict(n) for n in w.nodes], [dict(p) for p in w.pods] + [pod(1, labels={"app": "a69"})], w.provs, w.pdbs)
    return w


SEEDS = list(range(21000, 21040))


def w_wide_random(seed):
    """<= 300 nodes, <= 400 PDBs, 1-40 namespaces, 1-40 keys with 2-200 values each, at most 3 pods per node on average.  80 % of the pods carry the first key (`app`);
    60 % of the PDBs are matchLabels on it, the rest 1-3 expressions (In : NotIn : Exists : DoesNotExist = 6 : 1 : 2 : 1, In / NotIn sets of 1, 2, 3, min(V, 70) or V
    values); 2 % nil selectors, 0.5 % empty ones; 30 % allow a disruption."""
    rs = np.random.RandomState(seed)
    nss = [f"ns{i}" for i in range(int(rs.randint(1, 41)))]
    keys = ["app"] + [f"key{i}" for i in range(1, int(rs.randint(1, 41)))]
    nvals = [int(rs.randint(2, 201)) for _ in keys]
    n_nodes, n_pdbs = int(rs.randint(1, 301)), int(rs.randint(0, 401))
    n_pods = int(rs.randint(0, 3 * n_nodes + 1))
    nodes = []
    for _ in range(n_nodes):
        kw = dict(prov="p0" if rs.rand() < 0.6 else "p1", age=float(rs.uniform(0, 5000)))
        r = rs.rand()
        if r < 0.03:
            kw["nominated"] = True
        elif r < 0.06:
            kw["deletion_timestamp"] = True
        elif r < 0.09:
            kw["drop"] = [[R.CAPACITY_TYPE, R.ZONE, R.INITIALIZED, R.PROVISIONER_NAME][int(rs.randint(4))]]
        nodes.append(node(**kw))

    def value(k):
        return f"val{int(rs.randint(nvals[k]))}" if rs.rand() < 0.9 else f"stray{int(rs.randint(3))}"
    pods = []
    for _ in range(n_pods):
        labels = {}
        if rs.rand() < 0.8:
            labels["app"] = value(0)
        for k in range(1, len(keys)):
            if rs.rand() < min(0.4, 3.0 / len(keys)):
                labels[keys[k]] = value(k)
        if rs.rand() < 0.3:
            labels["pod-template-hash"] = f"h{int(rs.randint(1000))}"
        pods.append(pod(int(rs.randint(n_nodes)), ns=nss[int(rs.randint(len(nss)))], labels=labels, dne=bool(rs.rand() < 0.01),
                        dc=float(rs.uniform(-2.0 ** 31, 2.0 ** 31)) if rs.rand() < 0.5 else None, prio=int(rs.randint(-2 ** 31, 10 ** 9)) if rs.rand() < 0.3 else None))
    pdbs = []
    for _ in range(n_pdbs):
        r = rs.rand()
        if r < 0.02:
            s = None
        elif r < 0.025:
            s = sel()
        elif r < 0.625:
            s = sel({"app": f"val{int(rs.randint(nvals[0]))}"})
        else:
            ex = []
            for _ in range(int(rs.randint(1, 4))):
                k = int(rs.randint(len(keys)))
                op = ["In"] * 6 + ["NotIn"] + ["Exists"] * 2 + ["DoesNotExist"]
                op = op[int(rs.randint(10))]
                vs = []
                if op in ("In", "NotIn"):
                    cnt = [1, 2, 3, min(nvals[k], 70), nvals[k]][int(rs.randint(5))]
                    vs = [f"val{int(x)}" for x in rs.choice(nvals[k], size=min(cnt, nvals[k]), replace=False)]
                ex.append((keys[k], op, vs))
            s = sel(exprs=ex)
        pdbs.append(pdb(s, ns=nss[int(rs.randint(len(nss)))], allowed=int(rs.randint(1, 3)) if rs.rand() < 0.3 else 0))
    assert n_nodes <= 300 and n_pdbs <= 400 and n_pods <= 3 * n_nodes and len(nss) <= 40 and len(keys) <= 40 and max(nvals) <= 200
    deleting = [int(x) for x in rs.choice(n_nodes, size=min(n_nodes, int(rs.randint(0, 3))), replace=False)]
    return World(nodes, pods, provs(ttl0=int(rs.randint(1, 6000)) if rs.rand() < 0.7 else None, ttl1=int(rs.randint(1, 6000)) if rs.rand() < 0.3 else None), pdbs, deleting)


def mentioned(w):
    """key -> the values the world's selectors mention."""
    m = {}
    for b in w.pdbs:
        if b.selector is not None:
            for k, v in b.selector.match_labels.items():
                m.setdefault(k, set()).add(v)
            for e in b.selector.match_expressions:
                m.setdefault(e.key, set()).update(e.values)
    return m


WIDE = {"limit_values": TCC.w_limit_values, "limit_keys": TCC.w_limit_keys, "sets": w_sets, "keys": w_keys, "per_app": w_per_app,
        "ns_1": lambda: w_namespaces(1), "ns_2": lambda: w_namespaces(2), "ns_65": lambda: w_namespaces(65),
        "pods_255": lambda: w_pod_counts(255), "pods_256": lambda: w_pod_counts(256), "pods_257": lambda: w_pod_counts(257), "events_70": w_events_70}
WIDE.update({f"wide-random-{s}": (lambda s=s: w_wide_random(s)) for s in SEEDS})
WIDE.update({"narrow:" + n: f for n, f in WORLDS.items()})                     # item 1: every world of the narrow route's file, with the flag
STILL_REFUSED = {"unflagged:limit_values": (TCC.w_limit_values, -2, ["63", "62"]), "unflagged:limit_keys": (TCC.w_limit_keys, -2, ["17", "16"])}      # without the flag: as before
WIDE_REFUSED = {"wide:bad_block": (TCC.w_bad_block, -1, ["PDB 0"]), "wide:nan_cost": (TCC.w_nan_cost, -1, ["not finite"]), "wide:ttl_zero": (TCC.w_ttl_zero, -1, ["divides"]),
                "unknown_flag": (TCC.w_lifetime, -1, ["unknown flag bit"])}
# the sibling call: expiration and drift over worlds 5 and 6 and five random seeds; emptiness once
DEPROV_BASES = ["per_app", "ns_2", "ns_65"] + [f"wide-random-{s}" for s in SEEDS[1:6]]
DEPROV = {f"{m}:{b}": (m, b) for b in DEPROV_BASES for m in ("expiration", "drift")}
DEPROV["emptiness:per_app"] = ("emptiness", "per_app")
METHODS = {"expiration": D.EXPIRATION, "drift": D.DRIFT, "emptiness": D.EMPTINESS}
_BUILT = {}


def world(name):
    if name not in _BUILT:
        for table in (WIDE, STILL_REFUSED, WIDE_REFUSED):
            if name in table:
                f = table[name]
                _BUILT[name] = (f[0] if isinstance(f, tuple) else f)()
    return _BUILT[name]


def deprov_world(name):
    """A consolidation world under a deprovisioning method: creation times 100 .. 700 s ago against ttls of 300 / 500 s, every third node not drifted, every fifth empty
    node carries an emptiness timestamp."""
    if name not in _BUILT:
        m, base = DEPROV[name]
        w = world(base)
        nodes = []
        for i, n in enumerate(w.nodes):
            d = dict(n)
            d.update(creation=TDC.NOW - (i % 7 + 1) * 100 * TDC.S_NS, emptiness=TDC.NOW - 100 * TDC.S_NS if i % 5 == 0 else None, vd=None if i % 3 == 0 else D.DRIFTED)
            nodes.append(d)
        _BUILT[name] = TDC.dworld(METHODS[m], nodes, w.pods, TDC.dprovs(ttl0=300, ttl1=500, ttl_e0=30), w.pdbs, w.deleting, drift_enabled=True)
    return _BUILT[name]


# ---------------------------------------------------------------------------------------------------------------- the device side
def _poisoned(n):
    return TDC._poisoned(n)


def _plain(got):
    return TDC._plain(got)


def device_run(S, name):
    """One world on one backend through the Python mirror of the _ex calls.  Plain data out; a refusal comes back with its code, its message and whether the arrays are untouched."""
    from karpenter_core_amd.model import pdbs_to_block
    if name in DEPROV:
        return deprov_run(S, name)
    w = world(name)
    pr, pod_node = TCC.problem(w)
    parsed = S.ParsedProblem(pr)
    out = {}
    try:
        if w.events:
            info = parsed.apply_block(w.events, pod_node)
            out["applied"] = info["applied"]
            pod_node = None
        after = w.after or w
        block = pdbs_to_block(w.pdbs)
        if w.bad_block:
            block = dict(block, n_words=block["n_words"] - 1)
        arrays = _poisoned(max(1, len(after.nodes)))
        bit = S.KSH_CAND_WIDE_SELECTORS
        try:
            if name == "unknown_flag":
                S.KSH_CAND_WIDE_SELECTORS = 2          # the mirror passes this constant as `flags`: a bit the library does not know
            got = S.consolidation_candidates(parsed, pod_node, pdbs=block, deleting=w.deleting, out=arrays, wide_selectors=not name.startswith("unflagged:"), **TCC.call_inputs(S, after))
        except S.KSolveError as e:
            return dict(out, refused=[e.code, str(e)], untouched=TDC._untouched(arrays))
        finally:
            S.KSH_CAND_WIDE_SELECTORS = bit
        out.update(_plain(got))
        return out
    finally:
        parsed.close()


def deprov_run(S, name):
    from karpenter_core_amd.model import pdbs_to_block
    w = deprov_world(name)
    pr, pod_node = TCC.problem(w)
    parsed = S.ParsedProblem(pr)
    try:
        kw = dict(method=w.method, pod_node=pod_node, now_unix_nanos=w.now, drift_enabled=w.drift_enabled, pdbs=pdbs_to_block(w.pdbs), deleting=w.deleting, **TDC.call_inputs(S, w))
        return _plain(S.deprovisioning_candidates(parsed, wide_selectors=True, **kw))
    finally:
        parsed.close()


class _WithoutFlags:
    """The library's C entry point from before the _ex ones behind the _ex name: the mirror's call minus its `flags` argument (position `at`)."""
    def __init__(self, fn, at):
        self.fn, self.at = fn, at

    def __setattr__(self, k, v):
        if k == "argtypes":
            self.fn.argtypes = list(v[:self.at]) + list(v[self.at + 1:])
        else:
            object.__setattr__(self, k, v)

    def __call__(self, *a):
        assert a[self.at] == 0
        return self.fn(*a[:self.at], *a[self.at + 1:])


class _OldEntryPoints:
    def __init__(self, kh):
        self._kh = kh
        self.ksh_consolidation_candidates_ex = _WithoutFlags(kh.ksh_consolidation_candidates, 7)
        self.ksh_deprovisioning_candidates_ex = _WithoutFlags(kh.ksh_deprovisioning_candidates, 8)

    def __getattr__(self, k):
        return getattr(self._kh, k)


def flags0_run(S):
    """ksh_consolidation_candidates / ksh_deprovisioning_candidates (the functions as they were) against the _ex functions with flags 0, over test_deprovisioning_candidates.WORLDS:
    the same arrays, the same shape of ms."""
    from karpenter_core_amd.model import pdbs_to_block
    real = S.libs
    out = {}
    for name in TDC.WORLDS:
        w = TDC.world(name)
        pr, pod_node = TCC.problem(w)
        pr.daemonset_pods = [Pod(uid=f"ds-{i}", namespace="kube-system") for i in range(w.daemonsets)]
        parsed = S.ParsedProblem(pr)
        try:
            if w.events:
                parsed.apply_block(w.events, pod_node)
                pod_node = None
            a = w.after or w
            block = pdbs_to_block(w.pdbs)
            kw = dict(method=w.method, pod_node=pod_node, now_unix_nanos=w.now, drift_enabled=w.drift_enabled, pdbs=block, deleting=w.deleting, **TDC.call_inputs(S, a))
            cons = dict(TCC.call_inputs(S, a), pdbs=block, deleting=w.deleting)
            new = [S.deprovisioning_candidates(parsed, **kw), S.consolidation_candidates(parsed, pod_node, **cons)]
            try:
                ks, kh = real()
                S.libs = lambda: (ks, _OldEntryPoints(kh))
                old = [S.deprovisioning_candidates(parsed, **kw), S.consolidation_candidates(parsed, pod_node, **cons)]
            finally:
                S.libs = real
            out[name] = dict(same=[_plain(a) == _plain(b) for a, b in zip(new, old)], ms_keys=[sorted(a["ms"]) == sorted(b["ms"]) and len(a["ms"]) == 4 for a, b in zip(new, old)],
                             why=[int(x) for x in new[0]["why"]])
        finally:
            parsed.close()
    return out


# ---- the ksolve.h-level function, through ctypes: two nodes, three pods, two PDBs (k0 In [1, 3] in namespace 0; k1 Exists in namespace 1)
class _KsIn(ctypes.Structure):      # include/ksolve.h ks_candidates_inputs
    _fields_ = [(n, ctypes.c_uint32) for n in ("n_pods", "n_nodes", "n_pdbs", "n_keys")] + \
               [(n, ctypes.c_void_p) for n in ("pod_node", "pod_ns", "pod_flags", "pod_deletion_cost", "pod_priority", "pod_val", "pdb_ns", "pdb_allowed", "pdb_req_off", "pdb_req_key", "pdb_req_mask",
                                               "node_why", "node_age_seconds", "node_ttl_seconds", "node_pods_off", "node_pods")]


class _KsLists(ctypes.Structure):      # include/ksolve.h ks_selector_lists
    _fields_ = [("n_keys", ctypes.c_uint32), ("n_namespaces", ctypes.c_uint32)] + \
               [(n, ctypes.c_void_p) for n in ("key_n_values", "pod_label_off", "pod_label_key", "pod_label_val", "req_key", "req_op", "req_val_off", "req_val")]


class _KsOut(ctypes.Structure):      # include/ksolve.h ks_candidates_outputs
    _fields_ = [("n_candidates", ctypes.c_uint32), ("n_empty", ctypes.c_uint32)] + [(n, ctypes.c_void_p) for n in ("order", "empty", "why", "detail", "n_node_pods", "cost")]


OTHER = 0xFFFFFFFF
FLAT_VALID = dict(pod_node=[0, 1, 1], pod_ns=[0, 0, 1], pod_label_off=[0, 2, 3, 4], pod_label_key=[0, 1, 0, 1], pod_label_val=[3, OTHER, 2, 0], key_n_values=[4, 1],
                  pdb_ns=[0, 1], pdb_allowed=[0, 0], pdb_req_off=[0, 1, 2], req_key=[0, 1], req_op=[0, 2], req_val_off=[0, 2, 2], req_val=[1, 3], node_pods_off=[0, 1, 3], node_pods=[0, 1, 2],
                  n_keys=2, n_namespaces=2)
FLAT_BAD = {"flat:pod_offsets_descend": (dict(pod_label_off=[0, 3, 2, 4]), "pod label offsets"), "flat:pod_offsets_start": (dict(pod_label_off=[1, 2, 3, 4]), "start at 0"),
            "flat:value_offsets_descend": (dict(req_val_off=[0, 3, 2]), "value offsets"), "flat:pod_key_range": (dict(pod_label_key=[0, 2, 0, 1]), "label key out of range"),
            "flat:pod_value_range": (dict(pod_label_val=[4, OTHER, 2, 0]), "label value out of range"), "flat:pod_keys_unordered": (dict(pod_label_key=[1, 0, 0, 1], pod_label_val=[0, 3, 2, 0]), "must ascend"),
            "flat:pod_key_twice": (dict(pod_label_key=[0, 0, 0, 1]), "must ascend"), "flat:req_key_range": (dict(req_key=[2, 1]), "requirement key out of range"),
            "flat:req_value_range": (dict(req_val=[1, 4]), "value out of range"), "flat:values_unsorted": (dict(req_val=[3, 1]), "values must ascend"), "flat:values_twice": (dict(req_val=[3, 3]), "values must ascend"),
            "flat:operator": (dict(req_op=[4, 2]), "unknown operator 4"), "flat:in_without_values": (dict(req_op=[0, 0]), "need values"), "flat:exists_with_values": (dict(req_op=[2, 2]), "take none"),
            "flat:namespace_range": (dict(pod_ns=[0, 0, 2]), "namespace id out of range")}


def flat_run(S, name):
    ks, kh = S.libs()
    f = dict(FLAT_VALID)
    f.update(FLAT_BAD[name][0] if name in FLAT_BAD else {})
    u32 = lambda k: np.ascontiguousarray(np.asarray(f[k], dtype=np.uint32))
    a = {k: u32(k) for k in ("pod_ns", "pod_label_off", "pod_label_key", "pod_label_val", "key_n_values", "pdb_ns", "pdb_req_off", "req_key", "req_op", "req_val_off", "req_val", "node_pods_off", "node_pods")}
    a.update(pod_node=np.asarray(f["pod_node"], dtype=np.int32), pdb_allowed=np.asarray(f["pdb_allowed"], dtype=np.int32), pod_flags=np.zeros(3, dtype=np.uint32), dc=np.zeros(3, dtype=np.float64),
             prio=np.zeros(3, dtype=np.int32), why=np.zeros(2, dtype=np.uint32), age=np.zeros(2, dtype=np.float64), ttl=np.full(2, -1, dtype=np.int64))
    p = lambda k: a[k].ctypes.data
    inp = _KsIn(3, 2, 2, 0, p("pod_node"), p("pod_ns"), p("pod_flags"), p("dc"), p("prio"), None, p("pdb_ns"), p("pdb_allowed"), p("pdb_req_off"), None, None, p("why"), p("age"), p("ttl"),
                p("node_pods_off"), p("node_pods"))
    lists = _KsLists(f["n_keys"], f["n_namespaces"], p("key_n_values"), p("pod_label_off"), p("pod_label_key"), p("pod_label_val"), p("req_key"), p("req_op"), p("req_val_off"), p("req_val"))
    arrays = _poisoned(2)
    out = _KsOut(0, 0, *(arrays[k].ctypes.data for k in ("order", "empty", "why", "detail", "n_node_pods", "cost")))
    ks.ks_consolidation_candidates_lists_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    rc = ks.ks_consolidation_candidates_lists_host(ctypes.byref(inp), ctypes.byref(lists), ctypes.byref(out), 0, None)
    ks.ks_last_error.restype = ctypes.c_char_p
    if rc != 0:
        return dict(refused=[rc, ks.ks_last_error().decode()], untouched=TDC._untouched(arrays))
    return dict(why=[int(x) for x in arrays["why"]], detail=[int(x) for x in arrays["detail"]], order=[int(x) for x in arrays["order"][:out.n_candidates]])


def mirror_case():
    """test_consolidation_candidates.composition_case()'s snapshot and CandidateInfo with 70 one-per-value PDBs on the pods' own label key, the last of which guards the
    value the pods carry; and the reference's answer for it."""
    from karpenter_core_amd import consolidation as C
    snap, info, _ = TCC.composition_case()
    info = C.CandidateInfo(**dict(info.__dict__, pdbs=[pdb(sel({"my-label": f"v{i}"})) for i in range(69)] + [pdb(sel({"my-label": "a"}))]))
    prov = dict(name=snap.provisioner.name, types=[snap.instance_types[t].name for t in snap.provisioner.instance_types], enabled=True, ttl=1000)
    nodes = [dict(labels=n.labels, nominated=i in info.nominated, annotation=None, deletion_timestamp=False, age=info.node_age_seconds[i], left=False) for i, n in enumerate(snap.nodes)]
    wp = [pod(i, ns=p.namespace, labels=p.labels, dne=p.uid in info.do_not_evict, dc=info.deletion_cost.get(p.uid), prio=info.priority.get(p.uid)) for i, b in enumerate(snap.bound) for p in b]
    return snap, info, reference(World(nodes, wp, [prov], list(info.pdbs)))


def mirror_run(S):
    from karpenter_core_amd import consolidation as C
    snap, info, _ = mirror_case()
    out = {"wide": C.consolidation_candidates_dev(snap, info, wide_selectors=True)}
    try:
        C.consolidation_candidates_dev(snap, info)
        out["narrow"] = "answered"
    except S.KSolveError as e:
        out["narrow"] = [e.code, str(e)]
    out["wide"]["cost"] = [bits(c) for c in out["wide"]["cost"]]
    return json.loads(json.dumps(out, default=list))


CHILD = TCC.CHILD.replace("import test_consolidation_candidates as T", "import test_candidates_wide_selectors as T").replace('T.composition_run(S, name) if name == "composition" else T.device_run(S, name)', 'T.any_run(S, name)')
assert "import test_candidates_wide_selectors as T" in CHILD and "T.any_run(S, name)" in CHILD and "test_consolidation_candidates" not in CHILD, "the sibling's child script was reworded"


def any_run(S, name):
    if name == "mirror":
        return mirror_run(S)
    if name == "flags0":
        return flags0_run(S)
    if name.startswith("flat:"):
        return flat_run(S, name)
    return device_run(S, name)


ALL_JOBS = list(WIDE) + list(STILL_REFUSED) + list(WIDE_REFUSED) + list(DEPROV) + ["flat:valid"] + list(FLAT_BAD) + ["flags0", "mirror"]


def run_in_child(names, sim, tmp):
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    path = os.path.join(tmp, "jobs.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "names": names}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=1500)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        return {name: {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]} for name in names}
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return run_in_child(ALL_JOBS, True, str(tmp_path_factory.mktemp("wide_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return run_in_child(ALL_JOBS, bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("wide_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]
_REF = {}


def ref(name):
    if name not in _REF:
        _REF[name] = TDC.reference(deprov_world(name)) if name in DEPROV else reference(world(name))
    return _REF[name]


def _got(res, name):
    got = res[name]
    assert "error" not in got, got["error"]
    return got


def _same(got, want, name):
    assert "refused" not in got, (name, got)
    for k in ("why", "detail", "n_node_pods", "order", "empty"):
        assert got[k] == want[k], (name, k, [(i, a, b) for i, (a, b) in enumerate(zip(got[k], want[k])) if a != b][:5])
    assert got["cost"] == [bits(c) for c in want["cost"]], name


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_narrow_worlds_on_the_wide_route(request, backend):
    """Every handmade and random world of test_consolidation_candidates.WORLDS with the flag: reasons, details, pod counts, costs (bitwise), order, empty list."""
    res = request.getfixturevalue(backend)
    for n in WORLDS:
        _same(_got(res, "narrow:" + n), reference(TCC.world(n)), n)
    ev = _got(res, "narrow:events")
    assert ev["applied"] == 3 and ev["why"][2] == 13 and ev["why"][0] == 11


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_value_limit_is_answered(request, backend):
    """In over 63 values, the pod carries v0: refused without the flag, blocked by PDB 0 with it."""
    got = _got(request.getfixturevalue(backend), "limit_values")
    _same(got, ref("limit_values"), "limit_values")
    assert got["why"] == [11] and got["detail"] == [0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_key_limit_is_answered(request, backend):
    """17 keys: the reference's answer (the pod has no label: the nine matchLabels fail, the eight Exists fail)."""
    got = _got(request.getfixturevalue(backend), "limit_keys")
    _same(got, ref("limit_keys"), "limit_keys")
    assert got["why"] == [0]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(STILL_REFUSED))
def test_without_the_flag_the_limits_are_still_refused(request, backend, name):
    got = _got(request.getfixturevalue(backend), name)
    _, code, needles = STILL_REFUSED[name]
    assert got.get("refused") and got["refused"][0] == code, got
    for n in needles:
        assert n in got["refused"][1], got["refused"]
    assert got["untouched"]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["sets", "keys", "per_app", "ns_1", "ns_2", "ns_65", "pods_255", "pods_256", "pods_257"])
def test_matches_the_reference(request, backend, name):
    _same(_got(request.getfixturevalue(backend), name), ref(name), name)


def test_the_handmade_worlds_say_what_they_should():
    """CPU only, the reference's own answers: if these moved, the cases above would no longer test what their names say."""
    s = ref("sets")
    per = {}
    for i, p in enumerate(world("sets").pods):
        per.setdefault(p["ns"], []).append(s["why"][i])
    for size in SET_SIZES:
        assert per[f"in-{size}"] == [11, 11, 11, 0, 0, 0] and per[f"notin-{size}"] == [0, 0, 0, 11, 11, 11], size
    assert len(mentioned(world("sets"))["k"]) == 300
    k = ref("keys")
    assert len(mentioned(world("keys"))) == 40
    assert k["why"] == [0, 0, 11, 0, 11, 0, 11, 11, 11, 0, 11, 0, 11, 11, 11, 11, 11, 11], k["why"]
    assert [d for d in k["detail"] if d >= 0] == [3, 0, 0, 1, 1, 4, 0, 2, 1, 2, 0, 3], k["detail"]
    a = ref("per_app")
    assert all(a["detail"][i] == i and a["why"][i] == 11 for i in range(N_APPS) if i % 3 != 2)
    assert all(a["why"][i] == 0 for i in range(N_APPS) if i % 3 == 2 and i != 5) and a["detail"][5] == 301 and a["detail"][7] == 7
    assert a["why"][N_APPS:] == [11, 0, 11, 11] and a["detail"][N_APPS:] == [302, -1, 304, 304]
    for kk in (1, 2, 65):
        n = ref(f"ns_{kk}")
        w = world(f"ns_{kk}")
        # a pod x reports tier 1 (k + i; +1 past the lonely PDB at index k), a pod y tier 2, dealt in reverse: the lowest index is not the list's first unless the grouping keeps the order
        for i in range(kk):
            assert n["detail"][3 * i: 3 * i + 3] == [kk + i + 1, 2 * kk + 1 + (kk - 1 - i) % kk, -1], (kk, i)
        assert n["why"][3 * kk:] == [0, 0, 0] and w.pdbs[kk].namespace == "lonely"
    for n in (255, 256, 257):
        r = ref(f"pods_{n}")
        assert r["why"] == [0] * (n - 1) + [11] and r["detail"][-1] == 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_randomised_worlds(request, backend):
    """40 committed seeds against the reference."""
    res = request.getfixturevalue(backend)
    for s in SEEDS:
        _same(_got(res, f"wide-random-{s}"), ref(f"wide-random-{s}"), s)


def test_the_seeds_are_not_soft():
    """From the generator and the reference alone: enough seeds pass each old limit, and enough hold both a PDB-blocked node and a plain candidate."""
    keys = values = either = both = 0
    for s in SEEDS:
        m = mentioned(world(f"wide-random-{s}"))
        k, v = len(m) > 16, any(len(x) > 62 for x in m.values())
        keys, values, either = keys + k, values + v, either + (k or v)
        why = ref(f"wide-random-{s}")["why"]
        both += 11 in why and 0 in why
    assert either >= 20 and keys >= 10 and values >= 10 and both >= 30, (either, keys, values, both)


@pytest.mark.parametrize("backend", BACKENDS)
def test_after_events(request, backend):
    """A BIND through ksh_env_apply_block of a pod whose app is the 70th mentioned value, then the wide call with pod_node = NULL."""
    got = _got(request.getfixturevalue(backend), "events_70")
    _same(got, ref("events_70"), "events_70")
    assert got["applied"] == 1 and got["why"] == [0, 11] and got["detail"] == [-1, 69] and got["n_node_pods"] == [1, 2]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(DEPROV))
def test_the_sibling_call(request, backend, name):
    """Expiration and drift (emptiness once: it assigns no PDB code) with the flag against deprovisioning_ref."""
    got, want = _got(request.getfixturevalue(backend), name), ref(name)
    _same(got, want, name)
    assert got["n_in_result"] == want["n_in_result"]


def test_the_sibling_worlds_reach_the_pdb_code():
    for name in DEPROV:
        if not name.startswith("emptiness"):
            why = ref(name)["why"]
            assert 11 in why and 0 in why, name
    assert set(ref("emptiness:per_app")["why"]) == {16}      # every node has a pod: emptiness never reaches a PDB


@pytest.mark.parametrize("backend", BACKENDS)
def test_flags_zero_is_the_old_call(request, backend):
    """Over test_deprovisioning_candidates.WORLDS the _ex functions with flags 0 and the functions as they were give the same arrays and the same four ms entries."""
    got = _got(request.getfixturevalue(backend), "flags0")
    assert len(got) >= 10
    for name, r in got.items():
        assert r["same"] == [True, True] and r["ms_keys"] == [True, True], name
        assert r["why"] == TDC.ref(name)["why"], name


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(WIDE_REFUSED))
def test_refusals(request, backend, name):
    """An unknown flag bit, a truncated PDB block, a non-finite cost, a ttl of 0: invalid on the wide route too, nothing written."""
    got = _got(request.getfixturevalue(backend), name)
    _, code, needles = WIDE_REFUSED[name]
    assert got.get("refused") and got["refused"][0] == code, got
    for n in needles:
        assert n in got["refused"][1], got["refused"]
    assert got["untouched"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_flat_form(request, backend):
    """ks_consolidation_candidates_lists_host on arrays written by hand: pod 0 (k0 = 3) is a member of [1, 3]; pod 2 carries k1, which Exists asks for; then every
    malformed array is KS_ERR_INVALID with the poisoned outputs untouched."""
    res = request.getfixturevalue(backend)
    ok = _got(res, "flat:valid")
    assert ok == dict(why=[11, 11], detail=[0, 1], order=[]), ok
    for name, (_, needle) in FLAT_BAD.items():
        got = _got(res, name)
        assert got.get("refused") and got["refused"][0] == -1 and needle in got["refused"][1], (name, got)
        assert got["untouched"], name


@pytest.mark.parametrize("backend", BACKENDS)
def test_python_mirror(request, backend):
    """consolidation_candidates_dev(..., wide_selectors=True) over a busy_cluster snapshot with 70 PDBs on the pods' label key: the reference's answer; without the flag, refused."""
    got = _got(request.getfixturevalue(backend), "mirror")
    _, _, want = mirror_case()
    for k in ("why", "detail", "n_node_pods", "order", "empty"):
        assert got["wide"][k] == want[k], k
    assert got["wide"]["cost"] == [bits(c) for c in want["cost"]]
    assert 11 in want["why"] and 69 in want["detail"]
    assert got["narrow"][0] == -2 and "70" in got["narrow"][1] and "62" in got["narrow"][1]


def _c_program(tmp_path, libdir):
    exe = str(tmp_path / "cabi_usage_candidates_wide")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cabi_usage_candidates_wide.c"),
                           "-o", exe, "-L", libdir, "-lkshost", "-lksolve", "-Wl,-rpath," + libdir])
    w = World([node(), node(), node(), node(drop=[R.ZONE])], [pod(0, labels={"app": "a69"}), pod(1, labels={"app": "a1"}), pod(1, labels={"app": "a70"}), pod(2, labels={"app": "a0"}), pod(2)], provs())
    pr, pod_node = TCC.problem(w)
    f = tmp_path / "snapshot.ksp"
    f.write_text(pr.to_ksp())
    out = subprocess.run([exe, str(f)] + [str(int(x)) for x in pod_node], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    w.pdbs = [pdb(sel({"app": f"a{i}"}), allowed=1 if i == 1 else 0) for i in range(70)]
    want = reference(w)
    assert want["why"] == [11, 0, 11, 5] and want["detail"][0] == 69
    assert "order: " + " ".join(f"n{i}" for i in want["order"]) + "\n" in out.stdout, out.stdout
    for i in range(4):
        assert f"n{i}: why {want['why'][i]} detail {want['detail'][i]} pods {want['n_node_pods'][i]} cost {bits(want['cost'][i])}" in out.stdout, out.stdout
    refused = [l for l in out.stdout.splitlines() if l.startswith("refused: ")]
    assert len(refused) == 2 and "70" in refused[0] and "62" in refused[0] and "unknown flag bit" in refused[1], out.stdout


def test_c_abi_from_c_on_the_emulator(tmp_path):
    """tests/cabi_usage_candidates_wide.c as C99 with -Wall -Werror -pedantic, linked against the emulator build of the two libraries."""
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    _c_program(tmp_path, build_sim.build())


@pytest.mark.gpu
def test_c_abi_from_c(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    _c_program(tmp_path, os.path.join(ROOT, "karpenter_core_amd"))
