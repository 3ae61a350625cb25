"""The per-class device records -- ClsPlan and ClsBrief, built once per problem by ks_build_plans, ks_link_ev / ks_link_ev_wide and ks_link_plans
(karpenter_core_amd/csrc/ksolve.hip) -- against the oracle's model of them (oracle/oracle.cpp Scheduler::class_model: the very functions solve_spec_v2 and
solve_watermark_check run on, exported as oracle_py.class_model).  Both pack kernels take their shortcuts from these records: which pods one evaluation answers for
(`ev`), which pods may share a speculation round (`tmask` / `tfull` / `rmask` / `rsure` / `zmask` / `dyn` / `flags`), the watermark over the existing nodes (`mono`), the
fit-bitmap reuse (`eq`), and `overflow`, which turns a Solve into KS_ERR_UNSUPPORTED.  The records are read through FlatProblem.class_tables() (kshost.h
ksh_debug_classes); pods map to class rows through pod_classes(), never through order.  Every comparison is bit-exact.

Problems whose groups all exist from the start and number at most 64 (`total`): the model says everything, and the records must say the same -- the masks as multisets
of columns (no group numbering is assumed), `ev` as a partition that is never coarser than the model's (correctness) and, for classes that hold no list positions, never
finer (speed).  Problems with relaxable terms or more than 64 groups: the device may only be more careful than the model.

Every case runs twice: unmarked, on the emulator build of the kernels (tests/sim) in a child process, and marked `gpu`, on the device; one child process per backend.

One-past-the-limit classes: host/encode.cpp refuses a class with more than 12 touched keys, 24 topology items or 3 hostname items when it flattens the problem
(KS_ERR_UNSUPPORTED from ksh_open), so no device record of such a class can exist behind the C ABI; only the record list (KS_MAX_REC) reaches the device one past its
limit, and shows `overflow`.  ONE_PAST says which door refuses each."""
import copy
import json
import os
import subprocess
import sys

import pytest

from karpenter_core_amd import fake, workloads as W
from karpenter_core_amd.model import (Container, Expr, HostPort, LabelSelector, Pod, PodAffinityTerm, PreferredTerm, Problem, StateNode, Taint, Toleration,
                                      TopologySpreadConstraint, Volume, WeightedPodAffinityTerm, LABEL_CAPACITY_TYPE, LABEL_HOSTNAME, LABEL_INSTANCE_TYPE, LABEL_PROVISIONER,
                                      LABEL_ZONE, NO_SCHEDULE)
from oracle import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KS_ERR_UNSUPPORTED = -2
HOST, ZONE, CT = LABEL_HOSTNAME, LABEL_ZONE, LABEL_CAPACITY_TYPE
MASKS = ("tmask", "tfull", "rmask", "rsure", "zmask")
SCHEDULE_ANYWAY = "ScheduleAnyway"


# ---------------------------------------------------------------------------------------------------------------- building blocks
def pod(uid, labels=None, requests=None, **kw):
    return Pod(uid=uid, labels=dict(labels or {}), containers=[Container(requests=dict(requests or {"cpu": "100m", "memory": "64Mi"}), ports=kw.pop("ports", []))], **kw)


def sel(**labels):
    return LabelSelector(match_labels=labels)


def spread(key, skew, selector, when="DoNotSchedule"):
    return TopologySpreadConstraint(skew, key, when, selector)


def term(key, selector):
    return PodAffinityTerm(key, selector)


def problem(pods, prov_labels=None, prov_reqs=None, taints=None, nodes=None, types=5):
    its = fake.instance_types(types)
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its), labels=prov_labels, requirements=prov_reqs, taints=taints)], pods=pods,
                   nodes=nodes or [], extra_well_known=list(fake.EXTRA_WELL_KNOWN))


def state_node(name, its, zone="test-zone-1", taints=None):
    labels = {LABEL_PROVISIONER: "default", LABEL_INSTANCE_TYPE: its.name, CT: "on-demand", ZONE: zone, HOST: name, "karpenter.sh/initialized": "true"}
    return StateNode(name=name, labels=labels, taints=list(taints or []), available={"cpu": "3", "memory": "3Gi", "pods": "20"}, capacity=dict(its.capacity))


# ---------------------------------------------------------------------------------------------------------------- handmade: one rule at a time
def hm_tmask_hostname_anti_vs_spread():
    return problem([pod("anti", {"app": "a"}, anti_required=[term(HOST, sel(app="a"))]), pod("spread", {"app": "s"}, spread=[spread(HOST, 1, sel(app="s"))])])


def hm_tmask_hostname_affinity_vs_zone():
    return problem([pod("aff", {"app": "h"}, affinity_required=[term(HOST, sel(app="h"))]), pod("zone", {"app": "z"}, spread=[spread(ZONE, 1, sel(app="z"))])])


def hm_zmask():
    return problem([pod("skew1-self", {"app": "s1"}, spread=[spread(HOST, 1, sel(app="s1"))]), pod("skew1-other", {"app": "n1"}, spread=[spread(HOST, 1, sel(app="none"))]),
                    pod("skew2-self", {"app": "s2"}, spread=[spread(HOST, 2, sel(app="s2"))]), pod("anti", {"app": "x"}, anti_required=[term(HOST, sel(app="y"))])])


def hm_rsure():
    return problem([pod("no-filter", {"app": "e"}, spread=[spread(HOST, 1, sel(app="e"))]),
                    pod("filter", {"app": "f"}, node_selector={ZONE: "test-zone-1"}, spread=[spread(HOST, 1, sel(app="f"))]),
                    pod("owner", {"app": "o"}, anti_required=[term(HOST, sel(app="victim"))]), pod("victim", {"app": "victim"})])


def hm_dyn1_zone_requirement():
    return problem([pod("free", {"app": "a"}, spread=[spread(ZONE, 1, sel(app="a"))]),
                    pod("held", {"app": "b"}, node_selector={ZONE: "test-zone-2"}, spread=[spread(ZONE, 1, sel(app="b"))])])


def hm_dyn1_two_keys():
    return problem([pod("z0", {"app": "z0"}, spread=[spread(ZONE, 1, sel(app="z0"))]), pod("z1", {"app": "z1"}, spread=[spread(ZONE, 2, sel(app="z1"))]),
                    pod("c0", {"app": "c0"}, spread=[spread(CT, 1, sel(app="c0"))])])


def hm_dyn1_17_groups():
    return problem([pod(f"g{i:02d}", {"app": f"g{i}"}, spread=[spread(ZONE, 1, sel(app=f"g{i}"))]) for i in range(17)])


def hm_dyn1_nine_domains():
    racks = [f"rack-{i}" for i in range(9)]
    return problem([pod("rack", {"app": "r"}, spread=[spread("rack", 1, sel(app="r"))]), pod("zone", {"app": "z"}, spread=[spread(ZONE, 1, sel(app="z"))])],
                   prov_reqs=[Expr("rack", "In", racks)])


def hm_dyn2():
    return problem([pod("anti", {"app": "x"}, anti_required=[term(HOST, sel(app="y"))]), pod("spread", {"app": "s"}, spread=[spread(HOST, 1, sel(app="s"))]),
                    pod("aff", {"app": "h"}, affinity_required=[term(HOST, sel(app="h"))])])


def hm_mono():
    its = fake.instance_types(5)
    return problem([pod("well-known", node_selector={ZONE: "test-zone-1"}), pod("custom", node_selector={"team": "a"}),
                    pod("anti", {"app": "x"}, anti_required=[term(HOST, sel(app="y"))]), pod("spread", {"app": "s"}, spread=[spread(ZONE, 1, sel(app="s"))]),
                    pod("inverse-only", {"app": "y"})], prov_labels={"team": "a"}, nodes=[state_node("n-0", its[4]), state_node("n-1", its[4], "test-zone-2")])


def hm_flags():
    """(Volumes count only against a driver some existing node limits: without the node the flattening rightly drops them, and the pod is an ordinary one.)"""
    node = state_node("n-0", fake.instance_types(5)[4])
    node.volume_limits = {"csi-a": 2}
    return problem([pod("plain"), pod("ports", ports=[HostPort(8080)]), pod("volumes", volumes=[Volume("csi-a", "default/claim-1")])], nodes=[node])


# what the model must say of each handmade pod: the lengths of its masks ("n_*") and its scalar fields
HANDMADE = {
    "tmask_hostname_anti_vs_spread": (hm_tmask_hostname_anti_vs_spread, {
        "anti": {"n_tmask": 0, "n_tfull": 2, "n_zmask": 2, "eligible": 1}, "spread": {"n_tmask": 0, "n_tfull": 1, "n_zmask": 1, "eligible": 1}}),
    "tmask_hostname_affinity_vs_zone": (hm_tmask_hostname_affinity_vs_zone, {
        "aff": {"n_tmask": 1, "n_tfull": 1, "n_host": 1, "n_zmask": 0}, "zone": {"n_tmask": 1, "n_tfull": 1, "n_narrow": 1, "n_zmask": 0}}),
    "zmask": (hm_zmask, {"skew1-self": {"n_zmask": 1, "self": 1}, "skew1-other": {"n_zmask": 0, "self": 0}, "skew2-self": {"n_zmask": 0, "self": 1}, "anti": {"n_zmask": 1}}),
    "rsure": (hm_rsure, {"no-filter": {"n_rmask": 1, "n_rsure": 1}, "filter": {"n_rmask": 1, "n_rsure": 0}, "owner": {"n_rmask": 1, "n_rsure": 1}, "victim": {"n_rmask": 1, "n_rsure": 1, "n_host": 1}}),
    "dyn1_zone_requirement": (hm_dyn1_zone_requirement, {"free": {"dyn": 1, "self": 1, "max_skew": 1}, "held": {"dyn": 0}}),
    "dyn1_two_keys": (hm_dyn1_two_keys, {"z0": {"dyn": 1, "max_skew": 1}, "z1": {"dyn": 1, "max_skew": 2}, "c0": {"dyn": 0}}),
    "dyn1_17_groups": (hm_dyn1_17_groups, dict({f"g{i:02d}": {"dyn": 1} for i in range(16)}, g16={"dyn": 0})),
    "dyn1_nine_domains": (hm_dyn1_nine_domains, {"rack": {"dyn": 0, "n_narrow": 1}, "zone": {"dyn": 1}}),
    "dyn2": (hm_dyn2, {"anti": {"dyn": 2, "self": 0}, "spread": {"dyn": 2, "self": 1, "max_skew": 1}, "aff": {"dyn": 0, "n_host": 1}}),
    "mono": (hm_mono, {"well-known": {"watermark": 1}, "custom": {"watermark": 0}, "anti": {"watermark": 1, "n_host": 1}, "spread": {"watermark": 0},
                       "inverse-only": {"watermark": 1, "n_host": 1, "n_rmask": 1}}),
    "flags": (hm_flags, {"plain": {"eligible": 1}, "ports": {"eligible": 0}, "volumes": {"eligible": 0}}),
}


# ---------------------------------------------------------------------------------------------------------------- evaluation classes
def ev_replicas():
    """Six replicas that differ only in labels (a spread group of another pod selects none of them): one evaluation class."""
    return problem([pod(f"r{i}", {"app": f"replica-{i}"}) for i in range(6)] + [pod("other", {"app": "o"}, requests={"cpu": "200m"}, spread=[spread(ZONE, 1, sel(app="o"))])])


def ev_requests(names):
    """A base pod and, for every resource name but `pods` (a pod counts 1 whatever it asks), a pod that differs from it in that request only: whichever index the
    flattening gives a name, every other index 0 .. R - 1 is the only difference of one pair (R = 8: ks_link_ev; R = 12 and 16: ks_link_ev_wide, resources 8.. compared outside the plan record)."""
    res = W.WIDE_NAMES[:names]
    big = {n: "64" for n in res}
    big.update({"cpu": "96", "memory": "768Gi", "ephemeral-storage": "500Gi", "pods": "234"})
    its = [fake.new_instance_type(f"wide-{i}", resources=dict(big), architecture="amd64", operating_systems=["linux"]) for i in range(3)]
    base = {n: "1" for n in res}
    pods = [pod("base-a", requests=base), pod("base-b", {"app": "b"}, requests=base)] + [pod(f"d{k:02d}", requests=dict(base, **{n: "2"})) for k, n in enumerate(res) if n != "pods"]
    return Problem(instance_types=its, provisioners=[fake.provisioner("default", len(its))], pods=pods, extra_well_known=list(fake.EXTRA_WELL_KNOWN))


def ev_tolerations():
    t = Taint("dedicated", "gpu", NO_SCHEDULE)
    return problem([pod("exists", tolerations=[Toleration(key="dedicated", operator="Exists")]),
                    pod("equal", tolerations=[Toleration(key="dedicated", operator="Equal", value="gpu", effect=NO_SCHEDULE)]),
                    pod("all", tolerations=[Toleration(operator="Exists")]), pod("none"),
                    pod("wrong-value", tolerations=[Toleration(key="dedicated", operator="Equal", value="cpu")])], taints=[t])


def ev_selected_by_anti():
    return problem([pod("owner", {"app": "o"}, anti_required=[term(HOST, sel(app="web"))]), pod("selected", {"app": "web"}), pod("free", {"app": "db"})])


def ev_self_selecting():
    return problem([pod("self", {"app": "s"}, spread=[spread(ZONE, 1, sel(app="s"))]), pod("not-self", {"app": "t"}, spread=[spread(ZONE, 1, sel(app="s"))])])


def ev_list_positions():
    """Pairs of replicas that differ only in labels and hold a list in their plan -- host ports, volumes (against a node that limits the driver), a hostname
    selector: the model evaluates each pair alike; the device, which compares list POSITIONS, may keep them apart (FINER_EV)."""
    node = state_node("n-0", fake.instance_types(5)[4])
    node.volume_limits = {"csi-a": 2}
    pods = []
    for k in "ab":
        pods += [pod(f"ports-{k}", {"app": k}, ports=[HostPort(8080)]), pod(f"volumes-{k}", {"app": k}, volumes=[Volume("csi-a", "default/claim-1")]),
                 pod(f"hostname-{k}", {"app": k}, node_selector={HOST: "n-0"}), pod(f"plain-{k}", {"app": k})]
    return problem(pods, nodes=[node])


def ev_table(classes, kinds):
    """`classes` pods with distinct labels in `kinds` evaluation classes (kinds = classes: all distinct), for the interning table of ks_link_ev."""
    return problem([pod(f"t{i:03d}", {"app": f"l{i}"}, requests={"cpu": f"{100 + i % kinds}m", "memory": "64Mi"}) for i in range(classes)])


EV_CASES = {
    "ev_replicas": (ev_replicas, {}), "ev_requests_8": (ev_requests, {"names": 8}), "ev_requests_12": (ev_requests, {"names": 12}), "ev_requests_16": (ev_requests, {"names": 16}),
    "ev_tolerations": (ev_tolerations, {}), "ev_list_positions": (ev_list_positions, {}), "ev_selected_by_anti": (ev_selected_by_anti, {}), "ev_self_selecting": (ev_self_selecting, {}),
    "ev_table_31": (ev_table, {"classes": 31, "kinds": 31}), "ev_table_32": (ev_table, {"classes": 32, "kinds": 32}), "ev_table_33": (ev_table, {"classes": 33, "kinds": 33}),
    "ev_table_200_in_3": (ev_table, {"classes": 200, "kinds": 3}), "ev_table_200_distinct": (ev_table, {"classes": 200, "kinds": 200}),
}


# ---------------------------------------------------------------------------------------------------------------- relaxable terms, more than 64 groups
TWO_TERMS = [[Expr(ZONE, "In", ["test-zone-1"])], [Expr(CT, "In", ["on-demand"])]]      # relaxing drops the first term: the KEYS of a spread group's node filter change, so
RELAXED_TERMS = TWO_TERMS[1:]                                                              # the relaxed pod owns ANOTHER spread group, created when it relaxes


def rx_preferences():
    """Preferred pod affinity / anti-affinity, preferred node affinity, ScheduleAnyway spreads, and spreads under two required node-affinity terms: the groups of
    the relaxed forms of the last start inactive."""
    pref = [PreferredTerm(1, [Expr(ZONE, "In", ["test-zone-1"])])]
    pods = [pod("pa", {"app": "pa"}, affinity_preferred=[WeightedPodAffinityTerm(1, term(ZONE, sel(app="pa")))]),
            pod("pn", {"app": "pn"}, anti_preferred=[WeightedPodAffinityTerm(1, term(HOST, sel(app="pn")))]),
            pod("sa", {"app": "sa"}, spread=[spread(ZONE, 1, sel(app="sa"), SCHEDULE_ANYWAY)]),
            pod("zs", {"app": "zs"}, preferred_affinity=pref, spread=[spread(ZONE, 1, sel(app="zs"))]),
            pod("hs", {"app": "hs"}, preferred_affinity=pref, spread=[spread(HOST, 1, sel(app="hs"))]),
            pod("z2", {"app": "z2"}, required_affinity=TWO_TERMS, spread=[spread(ZONE, 1, sel(app="z2")), spread(HOST, 2, sel(app="zs"))]),
            pod("plain", {"app": "zs"})]
    return problem(pods)


def rx_late_hostname_group():
    """`late`: a hostname spread under two required node-affinity terms.  The relaxed pod owns another hostname spread group, which no node has registered with: a
    class that records into it -- `late` itself, `same-labels` -- must stay out of the rounds."""
    return problem([pod("late", {"app": "l"}, required_affinity=TWO_TERMS, spread=[spread(HOST, 1, sel(app="l"))]), pod("same-labels", {"app": "l"}), pod("plain")])


def rx_relaxed_form():
    """`late` of rx_late_hostname_group written directly in its relaxed form: the class of the later stage."""
    return problem([pod("late", {"app": "l"}, required_affinity=RELAXED_TERMS, spread=[spread(HOST, 1, sel(app="l"))]), pod("same-labels", {"app": "l"}), pod("plain")])


def rx_many_groups():
    """45 pods x (zone spread + hostname spread) with selectors of their own: 90 groups, bits alias as g & 63."""
    return problem([pod(f"m{i:02d}", {"app": f"m{i}", "tier": f"t{i % 5}"}, spread=[spread(ZONE, 1 + i % 2, sel(app=f"m{i}")), spread(HOST, 1, sel(tier=f"t{i % 5}", app=f"m{i}"))])
                    for i in range(45)])


RX_CASES = {"rx_preferences": (rx_preferences, {}), "rx_late_hostname_group": (rx_late_hostname_group, {}), "rx_relaxed_form": (rx_relaxed_form, {}), "rx_many_groups": (rx_many_groups, {})}
NOT_TOTAL = {"rx_preferences", "rx_late_hostname_group", "rx_many_groups"}


# ---------------------------------------------------------------------------------------------------------------- the limits of a plan
def _keyed(n):
    return {f"k{i:02d}": "v" for i in range(n)}


def lim_touch(n):
    """A class with own requirements on n narrow keys (labels every node of the template carries)."""
    return problem([pod("touch", node_selector=_keyed(n)), pod("plain")], prov_labels=_keyed(13))


def lim_topo(n):
    """A class that owns n zone spread groups (none selects it: its record list stays empty)."""
    return problem([pod("topo", {"app": "t"}, spread=[spread(ZONE, 3, sel(app=f"other-{i}")) for i in range(n)]), pod("other", {"app": "other-0"})])


def lim_host(n):
    return problem([pod("host", {"app": "h"}, anti_required=[term(HOST, sel(app=f"other-{i}")) for i in range(n)]), pod("other", {"app": "other-0"})])


def lim_rec(n):
    """`target` is selected by n zone spread groups that two other pods own; it owns none."""
    owners = [pod(f"owner-{j}", spread=[spread(ZONE, 4, sel(**{f"l{i:02d}": "y"})) for i in range(n) if i % 2 == j]) for j in range(2)]
    return problem(owners + [pod("target", {f"l{i:02d}": "y" for i in range(n)})])


def lim_touch_and_record():
    """12 touched keys of its own, and a record into a zone spread group: the thirteenth narrow key is not gathered into `touch` (PlanRec::tidx stays 0xFF)."""
    return problem([pod("touch", {"app": "w"}, node_selector=_keyed(12)), pod("spreader", spread=[spread(ZONE, 1, sel(app="w"))]), pod("plain", {"app": "w"})], prov_labels=_keyed(13))


AT_LIMIT = {"lim_touch_12": (lim_touch, {"n": 12}, "touch"), "lim_topo_24": (lim_topo, {"n": 24}, "topo"), "lim_host_3": (lim_host, {"n": 3}, "host"),
            "lim_rec_24": (lim_rec, {"n": 24}, "target"), "lim_touch_12_record_13th": (lim_touch_and_record, {}, "touch")}
# one past each limit -> (builder, arguments, the pod, which door refuses: "open" the flattening (ksh_open), "solve" the kernel through the record's `overflow`)
ONE_PAST = {"lim_touch_13": (lim_touch, {"n": 13}, "touch", "open"), "lim_topo_25": (lim_topo, {"n": 25}, "topo", "open"), "lim_host_4": (lim_host, {"n": 4}, "host", "open"),
            "lim_rec_25": (lim_rec, {"n": 25}, "target", "solve")}


# ---------------------------------------------------------------------------------------------------------------- batches
def bt_small():
    return problem([pod("a", {"app": "a"}, spread=[spread(ZONE, 1, sel(app="a"))]), pod("b", {"app": "a"}), pod("c", requests={"cpu": "300m"})])


def bt_many():
    return problem([pod(f"n{i:03d}", {"app": f"n{i % 7}"}, requests={"cpu": f"{100 + i % 44}m", "memory": "64Mi"}, spread=[spread(HOST, 1, sel(app=f"n{i}"))] if i % 13 == 0 else [])
                    for i in range(132)], types=20)


BATCH_MEMBERS = {"bt_small": (bt_small, {}), "bt_many": (bt_many, {}), "bt_wide_12": (ev_requests, {"names": 12})}
BATCHES = {"small_many_wide": ["bt_small", "bt_many", "bt_wide_12", "bt_small"], "wide_first": ["bt_wide_12", "bt_small", "bt_many"]}

CASES = {}
CASES.update({k: (v[0], {}) for k, v in HANDMADE.items()})
CASES.update(EV_CASES)
CASES.update(RX_CASES)
CASES.update({k: (v[0], v[1]) for k, v in AT_LIMIT.items()})
CASES.update({k: (v[0], v[1]) for k, v in ONE_PAST.items()})
CASES.update(BATCH_MEMBERS)
SOLVED = set(AT_LIMIT) | set(ONE_PAST)
# device classes that may be finer than the model's because they hold list positions (ports, volumes, hostname selector values): what the case's author expects
FINER_EV = {name: 0 for name in CASES}
FINER_EV["ev_list_positions"] = 3      # one split per pair: the two ports lists, the two volume lists and the two hostname lists each sit at a position of their own


def build_problem(name):
    fn, kw = CASES[name]
    return fn(**kw)


# ---------------------------------------------------------------------------------------------------------------- the device side
BRIEF_FIELDS = ("tmask", "tfull", "rmask", "ev", "flags", "reqmask", "dyn", "zmask", "rsure", "dyn_maxskew", "dyn_pd")
PLAN_FIELDS = ("present", "complement", "it_state", "hn_mode", "hn_off", "hn_cnt", "reqmask", "tol", "port_off", "port_cnt", "vol_off", "vol_cnt", "mono", "dyn", "ntouch", "ntopo",
               "nhost", "nrec", "tmask", "rmask", "overflow", "eq", "tkeys")


def tables_as_data(fp):
    """class_tables() as plain data: per class, every field of the brief and of the plan (the lists cut at their counts: what lies beyond is zero-filled)."""
    briefs, plans = fp.class_tables()
    out = []
    for c in range(fp.dims["C"]):
        b, p = briefs[c], plans[c]
        rec = {"b_" + f: int(getattr(b, f)) for f in BRIEF_FIELDS}
        rec.update({"p_" + f: int(getattr(p, f)) for f in PLAN_FIELDS})
        rec["b_req"], rec["p_req"], rec["p_c"] = [int(x) for x in b.req], [int(x) for x in p.req], int(p.c)
        rec["p_touch"] = [[int(t.mask), t.gt, t.lt, t.key, t.own, t.complement, t.topo_begin, t.topo_end] for t in p.touch[:min(p.ntouch, 12)]]
        rec["p_topo"] = [[int(t.PD), t.g, t.maxskew, t.type, t.self, t.pod_has, t.hslot] for t in p.topo[:min(p.ntopo, 24)]]
        rec["p_host"] = [[int(t.PD), t.g, t.maxskew, t.type, t.self, t.pod_has, t.hslot] for t in p.host[:min(p.nhost, 3)]]
        rec["p_rec"] = [[r.g, r.key, r.type, r.owned_inverse, r.hslot, r.tidx, r.filtered] for r in p.rec[:min(p.nrec, 24)]]
        out.append(rec)
    return out


def device_case(S, name, solve):
    try:
        fp = S.FlatProblem(build_problem(name))
    except S.KSolveError as e:
        return {"open_error": e.code}
    try:
        out = {"dims": dict(fp.dims), "cls": [int(c) for c in fp.pod_classes()], "res_names": fp.resource_names(), "first": tables_as_data(fp)}
        fp.grid()                                    # a second build of every static table, in place
        out["second"] = tables_as_data(fp)
        if solve:
            try:
                out["solve"] = fp.solve().canonical()
            except S.KSolveError as e:
                out["solve_error"] = e.code
        return out
    finally:
        fp.close()


def device_batch(S, members):
    """The tables a batched build leaves in every member: read with nothing rebuilt (class_tables() builds only what nothing has built)."""
    flats = [S.FlatProblem(build_problem(m)) for m in members]
    try:
        S.upload_batch(flats)
        S.solve_batch_resident(flats)
        return {"dims": [dict(f.dims) for f in flats], "tables": [tables_as_data(f) for f in flats]}
    finally:
        for f in flats:
            f.close()


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
job = json.loads(open(sys.argv[1]).read())
if job["sim"]:
    import simlib
    S = simlib.use_sim()
else:
    from karpenter_core_amd import scheduler as S
import test_class_tables as T
out = {"cases": {}, "batches": {}}
for name in job["cases"]:
    try:
        out["cases"][name] = T.device_case(S, name, name in T.SOLVED)
    except Exception as e:
        out["cases"][name] = {"error": repr(e)[:400]}
for name, members in job["batches"].items():
    try:
        out["batches"][name] = T.device_batch(S, members)
    except Exception as e:
        out["batches"][name] = {"error": repr(e)[:400]}
print("RESULT " + json.dumps(out))
"""


def all_results(sim, tmp):
    """Every case and every batch on one backend, in ONE fresh process."""
    env = dict(os.environ)
    env.pop("KS_TEST_SIM", None)
    path = os.path.join(tmp, "job.json")
    with open(path, "w") as fh:
        json.dump({"sim": sim, "cases": list(CASES), "batches": BATCHES}, fh)
    pr = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": HERE}, path], capture_output=True, text=True, env=env, timeout=900)
    line = [l for l in pr.stdout.splitlines() if l.startswith("RESULT ")]
    if not line:
        err = {"error": f"child exited {pr.returncode}\n" + pr.stdout[-2000:] + pr.stderr[-3000:]}
        return {"cases": {n: err for n in CASES}, "batches": {n: err for n in BATCHES}}
    return json.loads(line[-1][7:])


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return all_results(True, str(tmp_path_factory.mktemp("class_tables_emu")))


@pytest.fixture(scope="module")
def gpu(tmp_path_factory):
    return all_results(bool(os.environ.get("KS_TEST_SIM")), str(tmp_path_factory.mktemp("class_tables_gpu")))


BACKENDS = ["emu", pytest.param("gpu", marks=pytest.mark.gpu)]


# ---------------------------------------------------------------------------------------------------------------- the model side and the comparison
_MODELS = {}


def model_of(name):
    """(problem, class model) of a case: computed once, shared, never changed."""
    if name not in _MODELS:
        pr = build_problem(name)
        _MODELS[name] = (pr, O.class_model(pr))
    return _MODELS[name]


def by_uid(name):
    pr, model = model_of(name)
    return {p.uid: model["pods"][i] for i, p in enumerate(pr.pods)}


def has_hostname_selector(p):
    return HOST in p.node_selector or any(e.key == HOST for t in p.required_affinity for e in t)


def popcount(x):
    return bin(x).count("1")


def partition(ids):
    """The partition a list of ids induces on its positions, free of the ids themselves."""
    first = {}
    return [first.setdefault(x, i) for i, x in enumerate(ids)]


def columns(rows_by_mask, width):
    """rows_by_mask: for each of the five masks, per pod, an iterable of set bit positions.  -> the sorted non-zero columns of the stacked pods x width matrices."""
    col = [0] * width
    row = 0
    for rows in rows_by_mask:
        for bits in rows:
            for b in bits:
                col[b] |= 1 << row
            row += 1
    return sorted(c for c in col if c)


def bits_of(x):
    return [b for b in range(64) if (x >> b) & 1]


def compare(pr, model, dev, total, finer_allowed=0, tables="first"):
    """Every difference between the device's records (`dev`: one backend's result of the case) and the model, as a list of sentences.  total: the model says everything
    (every group initial, G <= 64); otherwise the device may only be more careful."""
    errs = []
    cls, recs, names = dev["cls"], dev[tables], dev["res_names"]
    mp = model["pods"]
    P = len(mp)
    assert len(cls) == P == len(pr.pods)
    rec = [recs[c] for c in cls]                                    # the device record of every pod
    for i in range(P):                                              # pods of one class must be one model class
        j = cls.index(cls[i])
        if j < i and {k: v for k, v in mp[i].items()} != {k: v for k, v in mp[j].items()}:
            errs.append(f"pods {j} and {i} share class {cls[i]} and differ in the model")
    # ---- ev: never coarser than the model
    dev_ev, mod_ev = [r["b_ev"] for r in rec], [m["ev"] for m in mp]
    seen = {}
    for i in range(P):
        j = seen.setdefault(dev_ev[i], i)
        if mod_ev[j] != mod_ev[i]:
            errs.append(f"ev soundness: pods {j} and {i} share ev {dev_ev[i]}, the model evaluates them differently")
    if total:
        # ---- masks: the same multiset of columns, the same popcounts
        dcols = columns([[bits_of(r["b_" + m]) for r in rec] for m in MASKS], 64)
        mcols = columns([[x[m] for x in mp] for m in MASKS], max(64, len(model["groups"])))
        if dcols != mcols:
            errs.append(f"masks: the columns differ: {len(dcols)} on the device, {len(mcols)} in the model; only there {[hex(c) for c in set(dcols) - set(mcols)][:4]}, only here {[hex(c) for c in set(mcols) - set(dcols)][:4]}")
        for m in MASKS:
            for i in range(P):
                if popcount(rec[i]["b_" + m]) != len(mp[i][m]):
                    errs.append(f"{m} of pod {i} ({pr.pods[i].uid}): {popcount(rec[i]['b_' + m])} bits on the device, {len(mp[i][m])} groups in the model")
        # ---- ev: for classes without list positions, never finer
        plain = [r["p_port_cnt"] == 0 and r["p_vol_cnt"] == 0 and r["p_hn_cnt"] == 0 for r in rec]
        finer = 0
        for e in sorted(set(mod_ev)):
            every = {dev_ev[i] for i in range(P) if mod_ev[i] == e}
            bare = {dev_ev[i] for i in range(P) if mod_ev[i] == e and plain[i]}
            if len(bare) > 1:
                errs.append(f"ev completeness: model class {e} (pods {[i for i in range(P) if mod_ev[i] == e][:6]}) is split into {len(bare)} on the device, none holds list positions")
            finer += len(every) - max(1, len(bare))
        if finer != finer_allowed:
            errs.append(f"ev: {finer} splits among classes that hold list positions, the case expects {finer_allowed}")
        # ---- the other fields
        for i in range(P):
            r, m, who = rec[i], mp[i], f"pod {i} ({pr.pods[i].uid})"
            if (r["b_flags"] & 1) != m["eligible"]:
                errs.append(f"{who}: flags {r['b_flags']}, eligible {m['eligible']}")
            if r["p_mono"] != m["watermark"]:
                errs.append(f"{who}: mono {r['p_mono']}, watermark {m['watermark']}")
            if (r["b_dyn"] & 3) != m["dyn"] or r["b_dyn"] != r["p_dyn"]:
                errs.append(f"{who}: dyn {r['b_dyn']:#x} (plan {r['p_dyn']:#x}), model {m['dyn']}")
            elif m["dyn"] == 1 and (((r["b_dyn"] >> 16) & 1) != m["self"] or r["b_dyn_maxskew"] != m["max_skew"]):
                errs.append(f"{who}: dyn 1 with self {(r['b_dyn'] >> 16) & 1} maxskew {r['b_dyn_maxskew']}, model {m['self']} / {m['max_skew']}")
            elif m["dyn"] == 2 and r["p_host"][0][3] == 0 and (r["p_host"][0][4] != m["self"] or r["p_host"][0][2] != m["max_skew"]):      # (self and maxSkew of a spread item: an anti-affinity item reads neither)
                errs.append(f"{who}: dyn 2 item {r['p_host'][0]}, model self {m['self']} maxskew {m['max_skew']}")
            if set(m["requests"]) - set(names):
                errs.append(f"{who}: requests {set(m['requests']) - set(names)} outside the resource names")
            want_mask = sum(1 << k for k, n in enumerate(names) if n in m["requests"])
            if r["b_reqmask"] != want_mask or r["p_reqmask"] != want_mask:
                errs.append(f"{who}: reqmask {r['b_reqmask']:#x} / {r['p_reqmask']:#x}, model {want_mask:#x}")
            want_req = [m["requests"].get(n, 0) for n in names[:8]] + [0] * (8 - min(8, len(names)))
            if r["b_req"] != want_req or r["p_req"] != want_req:
                errs.append(f"{who}: req {r['b_req']}, model {want_req}")
            if (r["p_ntopo"], r["p_nhost"], r["p_nrec"]) != (len(m["narrow"]), len(m["host"]), len(m["rmask"])):
                errs.append(f"{who}: ntopo / nhost / nrec {(r['p_ntopo'], r['p_nhost'], r['p_nrec'])}, model {(len(m['narrow']), len(m['host']), len(m['rmask']))}")
            p = pr.pods[i]
            want_eq = not (m["narrow"] or m["host"] or any(c.ports for c in p.containers) or p.volumes or has_hostname_selector(p))
            if (r["p_eq"] != 0) != want_eq:
                errs.append(f"{who}: eq {r['p_eq']}, the fit-bitmap reuse {'applies' if want_eq else 'does not apply'}")
        with_eq = [i for i in range(P) if rec[i]["p_eq"]]
        if partition([rec[i]["p_eq"] for i in with_eq]) != partition([dev_ev[i] for i in with_eq]):
            errs.append("eq and ev partition the classes without topology differently")
    else:
        pairs = (("tmask", "rmask"), ("tfull", "rmask"), ("zmask", "rsure"))
        for a, b in pairs:
            for i in range(P):
                for j in range(P):
                    if set(mp[i][a]) & set(mp[j][b]) and not rec[i]["b_" + a] & rec[j]["b_" + b]:
                        errs.append(f"{a} of pod {i} meets {b} of pod {j} in the model, not on the device")
        for i in range(P):
            if (rec[i]["b_flags"] & 1) and not mp[i]["eligible"]:
                errs.append(f"pod {i}: flags {rec[i]['b_flags']} where the model keeps the class out of the rounds")
            if rec[i]["p_mono"] and not mp[i]["watermark"]:
                errs.append(f"pod {i}: mono where the model has no watermark")
    return errs


IDENTITY = ("b_ev", "p_eq", "p_c")


def same_tables(a, b):
    """Two reads of one problem's tables: `ev` / `eq` as partitions (the member that represents a class may differ), everything else by value."""
    errs = []
    if len(a) != len(b):
        return [f"{len(a)} classes against {len(b)}"]
    for f in ("b_ev", "p_eq"):
        if partition([r[f] for r in a]) != partition([r[f] for r in b]) or [r[f] == 0 for r in a] != [r[f] == 0 for r in b]:
            errs.append(f"{f}: the partitions differ")
    for c, (x, y) in enumerate(zip(a, b)):
        diff = [k for k in x if k not in IDENTITY and x[k] != y[k]]
        if diff or x["p_c"] != y["p_c"]:
            errs.append(f"class {c}: {diff or ['p_c']} differ")
    return errs


def case_result(res, name):
    got = res["cases"][name]
    assert "error" not in got, got["error"]
    return got


# ---------------------------------------------------------------------------------------------------------------- tests
TOTAL_CASES = [n for n in list(HANDMADE) + list(EV_CASES) + list(RX_CASES) + list(AT_LIMIT) + list(BATCH_MEMBERS) if n not in NOT_TOTAL]


def test_the_cases_say_what_they_should():
    """(CPU) The model's answer for every handmade pod is what its case was written for; the other families hold what they are named after."""
    for name, (_, want) in HANDMADE.items():
        pr, model = model_of(name)
        assert all(g["initial"] or k >= model["inverse_from"] for k, g in enumerate(model["groups"])) and len(model["groups"]) <= 64
        got = by_uid(name)
        assert set(want) <= set(got), name
        for uid, fields in want.items():
            for f, v in fields.items():
                have = len(got[uid][f[2:]]) if f.startswith("n_") else got[uid][f]
                assert have == v, (name, uid, f, have, v)
    m = by_uid("tmask_hostname_affinity_vs_zone")
    assert m["aff"]["tmask"] == m["aff"]["host"] and m["zone"]["tmask"] == m["zone"]["narrow"]
    two = model_of("dyn1_two_keys")[1]
    assert sorted(g["key"] for g in two["groups"] if g["dyn"]) == [ZONE, ZONE] and sum(g["key"] == CT for g in two["groups"]) == 1
    assert sum(g["dyn"] for g in model_of("dyn1_17_groups")[1]["groups"]) == 16
    assert not any(g["dyn"] for g in model_of("dyn1_nine_domains")[1]["groups"] if g["key"] == "rack")
    # evaluation classes
    ev = lambda name: {u: x["ev"] for u, x in by_uid(name).items()}
    r = ev("ev_replicas")
    assert len({r[f"r{i}"] for i in range(6)}) == 1 and r["other"] != r["r0"]
    for names in (8, 12, 16):
        e = ev(f"ev_requests_{names}")
        assert e["base-a"] == e["base-b"] and len(e) == names + 1 and len(set(e.values())) == names
    t = ev("ev_tolerations")
    assert t["exists"] == t["equal"] == t["all"] and t["none"] == t["wrong-value"] != t["all"]
    a = ev("ev_selected_by_anti")
    assert len({a["owner"], a["selected"], a["free"]}) == 3
    s = ev("ev_self_selecting")
    assert s["self"] != s["not-self"] and by_uid("ev_self_selecting")["self"]["narrow"] == by_uid("ev_self_selecting")["not-self"]["narrow"]
    assert len(set(ev("ev_table_200_in_3").values())) == 3 and len(set(ev("ev_table_200_distinct").values())) == 200
    # relaxable terms: the relaxed form of `late` owns a hostname spread group of its own; more than 64 groups
    assert 80 <= len(model_of("rx_many_groups")[1]["groups"]) <= 130
    assert by_uid("rx_relaxed_form")["late"]["eligible"] == 1 and by_uid("rx_late_hostname_group")["late"]["eligible"] == 1      # (at stage 0 the model knows no late group)
    assert len(model_of("rx_late_hostname_group")[1]["groups"]) == 1
    # limits
    for name, (_, _, uid) in AT_LIMIT.items():
        m = by_uid(name)[uid]
        assert {"lim_touch_12": True, "lim_topo_24": len(m["narrow"]) == 24, "lim_host_3": len(m["host"]) == 3, "lim_rec_24": len(m["rmask"]) == 24 and not m["narrow"],
                "lim_touch_12_record_13th": len(m["rmask"]) == 1}[name], name
    for name, (_, _, uid, _) in ONE_PAST.items():
        m = by_uid(name)[uid]
        assert {"lim_touch_13": True, "lim_topo_25": len(m["narrow"]) == 25, "lim_host_4": len(m["host"]) == 4, "lim_rec_25": len(m["rmask"]) == 25}[name], name


def test_the_watermark_holds_for_a_hostname_selector():
    """(CPU) ClsPlan::mono is set for a class whose only requirement outside the well-known keys is on the hostname, and the model says the same: every existing node
    defines its hostname, so its refusal is final.  The dynamic check of the rule (oracle.cpp solve_watermark_check) over pods that fill the node they name: every pod is
    a watermark pod, refusals are on record and rechecked, none is taken back."""
    its = fake.instance_types(5)
    pods = [pod(f"h{i}", {"app": f"h{i % 2}"}, requests={"cpu": "1"}, node_selector={HOST: "n-0"}) for i in range(5)] + \
           [pod(f"x{i}", requests={"cpu": "1"}, required_affinity=[[Expr(HOST, "NotIn", ["n-0"])]]) for i in range(4)]
    pr = problem(pods, nodes=[state_node("n-0", its[4]), state_node("n-1", its[4], "test-zone-2")])
    assert all(m["watermark"] == 1 for m in O.class_model(pr)["pods"])
    res, ctr = O.watermark_check(pr)
    assert res.canonical() == O.solve(pr).canonical() and len(res.existing["n-0"]) == 3 and len(res.unscheduled) == 2
    assert ctr["violations"] == 0 and ctr["watermark_pods"] >= len(pods) and ctr["recorded_pairs_rechecked"] > 0


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", TOTAL_CASES)
def test_records_say_what_the_model_says(request, backend, case):
    """Masks as multisets of columns and by popcount, `ev` sound and complete, flags, mono, dyn, requests, the plan's counts, eq."""
    pr, model = model_of(case)
    got = case_result(request.getfixturevalue(backend), case)
    assert got["dims"]["G"] <= 64 and all(g["initial"] or k >= model["inverse_from"] for k, g in enumerate(model["groups"]))
    assert not compare(pr, model, got, True, FINER_EV[case])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", sorted(NOT_TOTAL))
def test_records_are_no_less_careful_than_the_model(request, backend, case):
    """Relaxable terms, more than 64 groups: every meet of the model's masks is a meet of the device's, flags and mono imply the model's, ev is sound."""
    pr, model = model_of(case)
    got = case_result(request.getfixturevalue(backend), case)
    assert not compare(pr, model, got, False)
    if case == "rx_many_groups":
        assert 80 <= got["dims"]["G"] <= 130
    else:
        assert got["dims"]["G"] > len(model["groups"]), "no group starts inactive: the case does not relax"


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_record_into_a_late_hostname_group_keeps_the_class_out_of_rounds(request, backend):
    res = request.getfixturevalue(backend)
    late = case_result(res, "rx_late_hostname_group")
    pr, _ = model_of("rx_late_hostname_group")
    uid = [p.uid for p in pr.pods]
    flags = lambda got, u: got["first"][got["cls"][uid.index(u)]]["b_flags"] & 1
    assert late["dims"]["G"] == 2 and (flags(late, "late"), flags(late, "same-labels"), flags(late, "plain")) == (0, 0, 1)
    relaxed = case_result(res, "rx_relaxed_form")      # the relaxed form, written directly: its group exists from the start
    assert relaxed["dims"]["G"] == 1 and (flags(relaxed, "late"), flags(relaxed, "same-labels"), flags(relaxed, "plain")) == (1, 1, 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", sorted(n for n in CASES if n not in ONE_PAST or ONE_PAST[n][3] != "open"))
def test_a_second_build_leaves_the_same_tables(request, backend, case):
    got = case_result(request.getfixturevalue(backend), case)
    assert not same_tables(got["first"], got["second"])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(AT_LIMIT))
def test_a_class_at_a_limit_fits_and_solves_like_the_oracle(request, backend, case):
    pr, model = model_of(case)
    got = case_result(request.getfixturevalue(backend), case)
    uid = AT_LIMIT[case][2]
    rec = got["first"][got["cls"][[p.uid for p in pr.pods].index(uid)]]
    assert rec["p_overflow"] == 0 and all(r["p_overflow"] == 0 for r in got["first"])
    want = {"lim_touch_12": ("p_ntouch", 12), "lim_topo_24": ("p_ntopo", 24), "lim_host_3": ("p_nhost", 3), "lim_rec_24": ("p_nrec", 24), "lim_touch_12_record_13th": ("p_ntouch", 12)}[case]
    assert rec[want[0]] == want[1]
    if case == "lim_touch_12_record_13th":
        assert rec["p_nrec"] == 1 and rec["p_rec"][0][5] == 0xFF and rec["p_rec"][0][1] not in [t[3] for t in rec["p_touch"]]
    assert "solve" in got, got.get("solve_error")
    assert json.loads(json.dumps(got["solve"])) == json.loads(json.dumps(O.solve(pr).canonical()))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", list(ONE_PAST))
def test_a_class_one_past_a_limit_is_refused_loudly(request, backend, case):
    """Refused with KS_ERR_UNSUPPORTED, by the door ONE_PAST names; where the record exists it says overflow and offers no shortcut."""
    pr, _ = model_of(case)
    got = case_result(request.getfixturevalue(backend), case)
    _, _, uid, door = ONE_PAST[case]
    if door == "open":
        assert got == {"open_error": KS_ERR_UNSUPPORTED}
        return
    rec = got["first"][got["cls"][[p.uid for p in pr.pods].index(uid)]]
    assert rec["p_overflow"] == 1 and rec["b_flags"] == rec["p_mono"] == rec["p_dyn"] == rec["b_dyn"] == rec["p_eq"] == 0
    assert sum(r["p_overflow"] for r in got["first"]) == 1
    assert "solve" not in got and got["solve_error"] == KS_ERR_UNSUPPORTED


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_a_batched_build_leaves_every_member_its_solo_tables(request, backend, batch):
    """Members with C = 3 beside C >= 130 and R <= 8 beside R = 12 (the batch links with ks_link_ev_wide): each member's tables, read with nothing rebuilt, are its own."""
    res = request.getfixturevalue(backend)
    got = res["batches"][batch]
    assert "error" not in got, got["error"]
    dims = got["dims"]
    assert min(d["C"] for d in dims) == 3 and max(d["C"] for d in dims) >= 130 and {d["R"] > 8 for d in dims} == {True, False} and max(d["R"] for d in dims) == 12
    for k, member in enumerate(BATCHES[batch]):
        solo = case_result(res, member)
        assert not same_tables(got["tables"][k], solo["first"]), (k, member)
        pr, model = model_of(member)
        assert not compare(pr, model, dict(solo, first=got["tables"][k]), True)


def test_the_comparison_can_fail(emu):
    """(CPU) Four ways a record can be wrong, made on a copy of the emulator's arrays of one handmade case: each is reported."""
    pr, model = model_of("rsure")
    got = case_result(emu, "rsure")
    assert not compare(pr, model, got, True)
    uid = [p.uid for p in pr.pods]
    cls = lambda u: got["cls"][uid.index(u)]

    def tampered(change):
        bad = copy.deepcopy(got)
        change(bad["first"])
        return compare(pr, model, bad, True)

    def set_mono(t):
        t[cls("no-filter")]["p_mono"] = 1

    def merge_ev(t):
        t[cls("filter")]["b_ev"] = t[cls("no-filter")]["b_ev"]

    def clear_tmask_bit(t):
        r = t[cls("victim")]
        assert r["b_tfull"]
        r["b_tfull"] &= r["b_tfull"] - 1

    def clear_rsure_bit(t):
        r = t[cls("owner")]
        assert r["b_rsure"]
        r["b_rsure"] &= r["b_rsure"] - 1

    assert any("mono" in e for e in tampered(set_mono))
    assert any("soundness" in e for e in tampered(merge_ev))
    assert any("tfull" in e or "columns" in e for e in tampered(clear_tmask_bit))
    assert any("rsure" in e for e in tampered(clear_rsure_bit))
    zone = copy.deepcopy(case_result(emu, "tmask_hostname_affinity_vs_zone"))
    pz, mz = model_of("tmask_hostname_affinity_vs_zone")
    r = zone["first"][zone["cls"][[p.uid for p in pz.pods].index("zone")]]
    assert r["b_tmask"]
    r["b_tmask"] &= r["b_tmask"] - 1
    assert any("tmask" in e for e in compare(pz, mz, zone, True))
