"""(CPU) What the Python binding of the audit's six passes (karpenter_core_amd/scheduler.py _AUDIT_PASSES) must not move:
  a) the layout of the ctypes mirrors of include/kshost.h's ksh_audit*_out -- tests and callers hand them to the C ABI directly --, size and every member's offset against
     what a C99 compiler says of the header.  Nothing is linked and no device is used;
  b) the shape of the dict each pass returns -- the keys, the type of every value, dtype and shape of the arrays, the names in the by-name counts -- over the smallest
     problem with a new node and an unscheduled pod (tests/audit_limits_cases.py's `capped` provisioner alone with five pods), on the emulator.
The expected keys are written out here, from the return statements of the binding before its six copies were folded into one table."""
import ctypes
import os
import subprocess

import pytest

import audit_harness as H
from karpenter_core_amd import scheduler as S

OUT = {"audit": ("ksh_audit_out", S._AuditOut), "topology": ("ksh_audit_topology_out", S._AuditTopologyOut), "spread": ("ksh_audit_spread_out", S._AuditSpreadOut),
       "firstfit": ("ksh_audit_firstfit_out", S._AuditFirstFitOut), "limits": ("ksh_audit_limits_out", S._AuditLimitsOut), "hostfit": ("ksh_audit_hostfit_out", S._AuditHostFitOut)}


@pytest.fixture(scope="module")
def header_layout(tmp_path_factory):
    """{struct: {"": sizeof, member: offsetof}} as gcc reads include/kshost.h, for the members the ctypes mirrors name."""
    lines = ['printf("%s  %%zu\\n", sizeof(%s));' % (c, c) for c, _ in OUT.values()]
    lines += ['printf("%s %s %%zu\\n", offsetof(%s, %s));' % (c, f[0], c, f[0]) for c, Out in OUT.values() for f in Out._fields_]
    d = tmp_path_factory.mktemp("layout")
    src, exe = str(d / "layout.c"), str(d / "layout")
    open(src, "w").write('#include <stdio.h>\n#include "kshost.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(H.ROOT, "include"), src, "-o", exe])
    got = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        c, member, n = line.split(" ")
        got.setdefault(c, {})[member] = int(n)
    return got


@pytest.mark.parametrize("what", list(OUT))
def test_the_struct_is_laid_out_as_the_header_says(header_layout, what):
    c, Out = OUT[what]
    mine = {"": ctypes.sizeof(Out)}
    mine.update({f[0]: getattr(Out, f[0]).offset for f in Out._fields_})
    assert mine == header_layout[c], (mine, header_layout[c])
    assert sum(ctypes.sizeof(f[1]) for f in Out._fields_) == ctypes.sizeof(Out)      # no padding: a member the mirror lacks would show as a hole, or in the size


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import numpy as np
import audit_limits_cases as LC
f = S.FlatProblem(LC.capped_problem(pods=5, second=False), flags=S.KS_FLAG_NO_RR)
f.solve(decode=False)
res, seq = f.result_arrays(), f.pod_seq()
assert f.dims["P"] == 5 and f.dims["E"] == 0 and res["n_new"] == 2, (f.dims, res["n_new"])
def shape(v):
    if isinstance(v, np.ndarray):
        return [str(v.dtype), list(v.shape)]
    if isinstance(v, dict):
        return {k: type(x).__name__ for k, x in v.items()}
    return [type(x).__name__ for x in v] if isinstance(v, tuple) else type(v).__name__
out = {}
for what in json.loads(sys.argv[1]):
    method = "audit" if what == "audit" else "audit_" + what
    forms = [getattr(f, method)(), getattr(f, method)(res) if what == "audit" else getattr(f, method)(res, seq), getattr(S, method + "_batch")([f])[0]]
    out[what] = [[[k, shape(v)] for k, v in d.items()] for d in forms]
f.close()
print("RESULT " + json.dumps(out))
"""

P, NODES = ["uint32", [5]], ["uint32", [2]]      # five pods; no existing node and two new ones
MS = ["float", "float"]


def _by_name(*names):
    return {k: "int" for k in names}


SEQ_BITS = {"topology": _by_name("SEQ", "ANTI_AFFINITY", "AFFINITY", "HOSTNAME_SPREAD"), "spread": _by_name("SEQ", "SPREAD"),
            "firstfit": _by_name("SEQ", "FIT_EXISTING", "FIT_NEW", "FIT_TEMPLATE"), "hostfit": _by_name("SEQ", "HFIT_EXISTING", "HFIT_NEW", "HFIT_TEMPLATE")}
EXPECTED = {
    "audit": [["pod_flags", P], ["node_flags", NODES], ["n_pods_flagged", "int"], ["n_nodes_flagged", "int"],
              ["pod_bit_count", _by_name("RANGE", "UNSCHEDULED_LIST", "TAINTS", "REQUIREMENTS", "HOSTNAME", "PORTS", "VOLUME_ERROR")],
              ["node_bit_count", _by_name("RESOURCES", "VOLUMES", "EMPTY", "TEMPLATE", "REQUESTS", "OPTIONS_EMPTY", "OPTIONS_EXTRA", "OPTIONS_MISSING")],
              ["n_new", "int"], ["n_unscheduled", "int"], ["ms", MS]],
    "topology": [["pod_flags", P], ["n_pods_flagged", "int"], ["pod_bit_count", SEQ_BITS["topology"]], ["checked", _by_name("SEQ", "ANTI_AFFINITY", "AFFINITY", "HOSTNAME_SPREAD")],
                 ["skipped_groups", "int"], ["n_new", "int"], ["n_placed", "int"], ["ms", MS]],
    "spread": [["pod_flags", P], ["n_pods_flagged", "int"], ["pod_bit_count", SEQ_BITS["spread"]], ["checked", _by_name("SEQ", "SPREAD")],
               ["exact_pairs", "int"], ["skipped_groups", "int"], ["n_new", "int"], ["n_placed", "int"], ["ms", MS]],
    "firstfit": [["pod_flags", P], ["n_pods_flagged", "int"], ["pod_bit_count", SEQ_BITS["firstfit"]], ["checked", _by_name("SEQ", "PODS", "PAIRS")],
                 ["admitting_pairs", "int"], ["skipped_pods", "int"], ["n_new", "int"], ["n_placed", "int"], ["ms", MS]],
    "limits": [["pod_flags", P], ["node_flags", NODES], ["n_pods_flagged", "int"], ["n_nodes_flagged", "int"], ["pod_bit_count", _by_name("SEQ", "LIMIT_TEMPLATE")],
               ["node_bit_count", _by_name("LIMIT_EXTRA", "LIMIT_MISSING")], ["checked", _by_name("SEQ", "NODES", "PODS", "PAIRS")], ["limited_templates", "int"],
               ["exact_nodes", "int"], ["binding_nodes", "int"], ["skipped_nodes", "int"], ["skipped_pods", "int"], ["n_new", "int"], ["n_placed", "int"], ["ms", MS]],
    "hostfit": [["pod_flags", P], ["n_pods_flagged", "int"], ["pod_bit_count", SEQ_BITS["hostfit"]], ["checked", _by_name("SEQ", "PODS", "PAIRS", "TESTS")],
                ["admitting_pairs", "int"], ["skipped_pods", "int"], ["eligible_groups", "int"], ["skipped_groups", "int"], ["n_new", "int"], ["n_placed", "int"], ["ms", MS]],
}


@pytest.fixture(scope="module")
def returned():
    return H.run_emulated(CHILD, list(EXPECTED))


@pytest.mark.parametrize("what", list(EXPECTED))
def test_the_dict_a_pass_returns_keeps_its_shape(returned, what):
    """The resident form, the claimed form and the batch form return the same keys in the same order, every value of the type and -- an array -- the dtype and shape it had."""
    for form, got in zip(("resident", "claimed", "batch"), returned[what]):
        assert got == EXPECTED[what], (form, got)
