"""(CPU) What the wide gate's ABI and its Python binding must not move -- tests/test_audit_stages_binding.py's method:
  a) the layout of the ctypes mirror of include/kshost.h's ksh_audit_gate_ex_out, size and every member's offset against what a C99 compiler says of the header; the
     growth rule's shape -- struct_size leads, the two new passes' pointers are the LAST members, everything ksh_audit_gate_out carries lies before them in its order;
  b) include/ksolve.h's ks_audit_gate_ex the same way (tests/test_audit_gate_ex_refusals.py builds it by hand from these offsets), and the three new defines;
  c) the pinned Python tables are unchanged: _AUDIT_PASSES, _AUDIT_PASSES_BESIDE, _AUDIT_PASSES_REASONS, KS_AUDIT_PASS (six names), _AuditGateOut, and the default
     `passes=None` of audit_gate still means the six and the old entry point;
  d) KS_AUDIT_PASS_EX and AUDIT_GATE_ALL: eight names, in mask order."""
import ctypes
import inspect
import os
import subprocess

import pytest

import audit_harness as H
from karpenter_core_amd import scheduler as S

KS_GATE_EX = ["struct_size", "passes", "cap_findings", "pad", "findings", "first", "topology", "spread", "firstfit", "limits", "hostfit", "first_pod_seq", "n_findings", "truncated",
              "kernel_ms", "readback_ms", "stages", "reasons"]
KS_GATE = ["passes", "cap_findings", "findings", "first", "topology", "spread", "firstfit", "limits", "hostfit", "first_pod_seq", "n_findings", "truncated", "kernel_ms", "readback_ms"]


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    lines = []
    for c_name, fields in (("ksh_audit_gate_ex_out", [f[0] for f in S._AuditGateExOut._fields_]), ("ksh_audit_gate_out", [f[0] for f in S._AuditGateOut._fields_]),
                           ("ks_audit_gate_ex", KS_GATE_EX), ("ks_audit_gate", KS_GATE)):
        lines += ['printf("%s. %%zu\\n", sizeof(%s));' % (c_name, c_name)] + ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f) for f in fields]
    lines += ['printf("%s %%u\\n", (unsigned)%s);' % (m, m) for m in ("KS_AUDIT_PASS_STAGES", "KS_AUDIT_PASS_REASONS", "KS_AUDIT_PASS_ALL_EX", "KS_AUDIT_PASS_ALL")]
    d = tmp_path_factory.mktemp("layout")
    src, exe = str(d / "layout.c"), str(d / "layout")
    open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include "ksolve.h"\n#include "kshost.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(H.ROOT, "include"), src, "-o", exe])
    return {line.split(" ")[0]: int(line.split(" ")[1]) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()}


def _mirror(Out, c_name):
    mine = {c_name + ".": ctypes.sizeof(Out)}
    mine.update({c_name + "." + f[0]: getattr(Out, f[0]).offset for f in Out._fields_})
    return mine


def test_the_wide_out_struct_is_laid_out_as_the_header_says(header):
    Out = S._AuditGateExOut
    mine = _mirror(Out, "ksh_audit_gate_ex_out")
    assert mine == {k: v for k, v in header.items() if k.startswith("ksh_audit_gate_ex_out.")}, (mine, header)
    assert sum(ctypes.sizeof(f[1]) for f in Out._fields_) == ctypes.sizeof(Out)      # no padding holes
    names = [f[0] for f in Out._fields_]
    assert names == ["struct_size", "pad", "findings", "cap_findings", "audit", "topology", "spread", "firstfit", "limits", "hostfit", "n_findings", "truncated", "stages", "reasons"]
    # the growth rule: the size leads, the later passes' pointers end the struct, and what the old struct carries keeps its order before them
    assert Out.struct_size.offset == 0 and names[-2:] == ["stages", "reasons"] and Out.reasons.offset + 8 == ctypes.sizeof(Out)
    assert [n for n in names if n not in ("struct_size", "pad", "stages", "reasons")] == [f[0] for f in S._AuditGateOut._fields_]


def test_the_old_out_struct_has_not_moved(header):
    assert _mirror(S._AuditGateOut, "ksh_audit_gate_out") == {k: v for k, v in header.items() if k.startswith("ksh_audit_gate_out.")}
    assert ctypes.sizeof(S._AuditGateOut) == 72 and header["ks_audit_gate."] == 96 and [header["ks_audit_gate." + f] for f in KS_GATE] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 88]


def test_libksolves_wide_struct_and_the_defines(header):
    assert header["ks_audit_gate_ex."] == 120 and header["ks_audit_gate_ex.struct_size"] == 0
    assert [header["ks_audit_gate_ex." + f] for f in KS_GATE_EX] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 84, 88, 96, 104, 112]
    assert (header["KS_AUDIT_PASS_STAGES"], header["KS_AUDIT_PASS_REASONS"], header["KS_AUDIT_PASS_ALL_EX"], header["KS_AUDIT_PASS_ALL"]) == (64, 128, 255, 63)


def test_the_pinned_python_tables_are_unchanged():
    assert list(S._AUDIT_PASSES) == ["audit", "topology", "spread", "firstfit", "limits", "hostfit"]
    assert list(S._AUDIT_PASSES_BESIDE) == ["stages"] and list(S._AUDIT_PASSES_REASONS) == ["reasons"]
    assert S.KS_AUDIT_PASS == {"audit": 1, "topology": 2, "spread": 4, "firstfit": 8, "limits": 16, "hostfit": 32}
    assert [f[0] for f in S._AuditGateOut._fields_] == ["findings", "cap_findings", "audit", "topology", "spread", "firstfit", "limits", "hostfit", "n_findings", "truncated"]
    sig = inspect.signature(S.audit_gate)
    assert sig.parameters["passes"].default is None and list(sig.parameters)[:6] == ["flats", "passes", "cap_findings", "claimed", "pod_seq", "findings_table"]
    assert inspect.signature(S.FlatProblem.audit_gate).parameters["passes"].default is None


def test_the_eight_names_in_mask_order():
    assert S.AUDIT_GATE_ALL == ("audit", "topology", "spread", "firstfit", "limits", "hostfit", "stages", "reasons")
    assert S.KS_AUDIT_PASS_EX == {"audit": 1, "topology": 2, "spread": 4, "firstfit": 8, "limits": 16, "hostfit": 32, "stages": 64, "reasons": 128}
    assert {k: v for k, v in S.KS_AUDIT_PASS_EX.items() if k in S.KS_AUDIT_PASS} == S.KS_AUDIT_PASS and sum(S.KS_AUDIT_PASS_EX.values()) == 255


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import audit_topo_cases as TC
(_,) = json.loads(sys.argv[1])
f = S.FlatProblem(TC.plain(3, True)); f.solve(decode=False)
calls = []
ks, kh = S.libs()
class Spy:
    def __init__(self, lib): self.lib = lib
    def __getattr__(self, name):
        if name.startswith("ksh_audit_gate"): calls.append(name)
        return getattr(self.lib, name)
real = S.libs
S.libs = lambda: (ks, Spy(kh))
default = S.audit_gate([f]); named = S.audit_gate([f], ["reasons", "audit", "stages"]); one = f.audit_gate(passes=["hostfit", "stages"])
S.libs = real
out = {"calls": calls, "default": list(default["passes"]), "named": list(named["passes"]), "one": list(one["passes"]), "clean": [default["clean"], named["clean"], one["clean"]]}
try:
    S.audit_gate([f], ["stages", "nonesuch"])
    out["unknown name"] = None
except KeyError as e:
    out["unknown name"] = str(e)
f.close()
print("RESULT " + json.dumps(out))
"""


def test_the_default_is_the_six_through_the_old_entry_point_and_passes_come_back_in_mask_order():
    got = H.run_emulated(CHILD, [0])
    assert got["calls"] == ["ksh_audit_gate", "ksh_audit_gate_ex", "ksh_audit_gate_ex"], got
    assert got["default"] == list(S._AUDIT_PASSES) and got["named"] == ["audit", "stages", "reasons"] and got["one"] == ["hostfit", "stages"] and got["clean"] == [True] * 3, got
    assert got["unknown name"] == "'nonesuch'", got
