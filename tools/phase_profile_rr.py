#!/usr/bin/env python3
"""Round statistics of the register-resident pack kernel (ks_pack_rr) on config #3 and, with a KS_PROBES build, where a round's cycles go.
The statistics slots of worker 1 hold the phases of a NORMAL round in a plain -DKS_PROBES build and the phases of a RUN round's step in a
-DKS_PROBES -DKS_PROBES_RUN one; the library says which it is (ks_probe_build), and only the rows that its counters are get printed.
usage: tools/phase_profile_rr.py [pods]"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from karpenter_core_amd import scheduler as S, workloads as W

pods = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
if os.environ.get("KS_VARIANT"):      # an experiment build under karpenter_core_amd/_variants/<name> (e.g. a -DKS_PROBES one) instead of the library in the tree
    S._HERE = os.path.join(os.path.dirname(S.__file__), "_variants", os.environ["KS_VARIANT"]); S._LIBS = None; S.libs()
ks = S.libs()[0]
try:
    ks.ks_probe_build.restype = ctypes.c_uint32
    build = int(ks.ks_probe_build())
except AttributeError:      # (a library from before ks_probe_build: nothing says what its slots hold)
    build = None
PROBES, WIN, RUN = 1, 2, 4      # include/ksolve.h: KS_PROBE_BUILD_*
pr = W.config3(pods=pods)
fp = S.FlatProblem(pr)
fp.upload(0)
fp.grid(want_bits=False)
fp.solve(decode=False)
r = fp.solve()
st = r.stats
tot = st["kernel_cycles"]
rounds = max(st["eq_pods"], 1)
print("kernel_ms", fp.kernel_ms, "nodes", len(r.new_nodes), "cycles", tot, "per pod", tot / pods)
print("rounds", st["eq_pods"], "evaluating", st["reuse_exhausted"], "bubbles", st["reuse_seeds"], "phase A runs", st["reuse_hits"],
      *(() if build and build & PROBES else ("nrcs", st["cyc_pop"], "exact checks", st["cyc_stage"])))      # (a probe build counts cycles in these two slots)
print("dyn1 answers", st.get("full_fails"), "| runs", st.get("p24"), "pods in runs", st.get("p22"), "steps", st.get("p23"))
pr_, pn = st.get("relaxations", 0) >> 32, st.get("relaxations", 0) & 0xFFFFFFFF
steps = max(st.get("p23", 0), 1)
LEADER = [("leader: form the batch (rest)", "cyc_evalout"), ("leader: wait at B1", "cyc_full"), ("leader: prepare entries", "cyc_commit"), ("leader: picks / run steps", "cyc_order"),
          ("leader: resolve", "cyc_new")]
if build is None or not build & PROBES:
    print("not a KS_PROBES build" if build is not None else "the library does not say which probes it was built with (no ks_probe_build): no phase rows")
elif build & WIN:
    print("a KS_PROBES_WIN build: its slots are the head window's (tools/win_profile.py)")
elif build & RUN:
    # worker 1's slots are the phases of a RUN round's step (RRT(0..7)); the leader's `run records` / `after records` slots (25, 26) hold two of them
    for nm, k in LEADER + [("worker 1: round tail (incl. runs)", "scan_chunks"), ("worker 1: wait at B1", "n_kind2")]:
        print(f"{nm:32s} {st.get(k, 0) / rounds:9.0f} cycles / round")
    print("raw:", {k: v for k, v in st.items() if v})
    print("run rounds: %d pods, %.0f cycles/pod | normal rounds: %d pods" % (pr_, st.get("attempts", 0) / max(pr_, 1), pn))
    run_rows = (("before the first step (once a run)", "cyc_pop"), ("group of equal items (rr_run_group)", "cyc_stage"), ("items change: masks again", "p25"), ("keys of the accepting slots", "p26"),
                ("extraction (publish)", "cyc_kind0"), ("barrier wait", "cyc_kind1"), ("merge", "cyc_kind2"), ("commit + retry", "n_kind1"))
    tot_run = sum(st.get(k, 0) for _, k in run_rows)
    for nm, k in run_rows:
        print(f"  run step: {nm:44s} {st.get(k, 0):11d} cycles {st.get(k, 0) / steps:9.0f} / step")
    print(f"  run step: {'worker 1, all of the above':44s} {tot_run:11d} cycles {tot_run / steps:9.0f} / step   (a KS_PROBES_RUN build; the leader's cycles in the steps -- p25 -- are a plain KS_PROBES build's)")
else:
    for nm, k in LEADER + [("leader: run records", "p25"), ("leader: after records", "p26"), ("worker 1: round tail (incl. runs)", "scan_chunks"),
                           ("worker 1: B1 wait", "cyc_kind0"), ("worker 1: between pods (commit, loop)", "cyc_kind1"), ("worker 1: EVAL", "cyc_kind2"), ("worker 1: candidate + atomic", "n_kind1"),
                           ("worker 1: barrier", "n_kind2"), ("worker 1: decide", "cyc_pop")]:
        print(f"{nm:40s} {st.get(k, 0) / rounds:9.0f} cycles / round")
    print("raw:", {k: v for k, v in st.items() if v})
    print("run rounds: %d pods, %.0f cycles/pod | normal rounds: %d rounds, %d pods, %.0f cycles/pod, %.0f cycles/round" % (pr_, st.get("attempts", 0) / max(pr_, 1), st.get("n_kind2", 0), pn, st.get("types_scanned", 0) / max(pn, 1), st.get("types_scanned", 0) / max(st.get("n_kind2", 0), 1)))
    print("cycles in RUN rounds (leader, `attempts`) %d | in their steps (leader, `p25`) %d" % (st.get("attempts", 0), st.get("p25", 0)))
    print("(the phases of a RUN round's step -- extraction | barrier | merge | commit + retry -- need a -DKS_PROBES -DKS_PROBES_RUN build: this one's worker slots are a normal round's)")
