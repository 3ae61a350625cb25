"""(CPU) What the Python binding of the audit's eighth pass (karpenter_core_amd/scheduler.py _AUDIT_PASSES_REASONS) must not move -- tests/test_audit_binding.py's
method for the new struct only:
  a) the layout of the ctypes mirror of include/kshost.h's ksh_audit_reasons_out, size and every member's offset against what a C99 compiler says of the header;
  b) the shape of the dict the pass returns in resident, claimed and batch form, over the smallest problem with a new node and an unscheduled pod, on the emulator;
  c) the table of its own leaves _AUDIT_PASSES and _AUDIT_PASSES_BESIDE, and with them the gate's mask bits and struct, as they were;
  d) the bits and the KS_WHY_* values are the header's."""
import ctypes
import os
import re
import subprocess

import pytest

import audit_harness as H
import test_audit_binding as TB
from karpenter_core_amd import scheduler as S

C_NAME, Out = "ksh_audit_reasons_out", S._AuditReasonsOut


@pytest.fixture(scope="module")
def header_layout(tmp_path_factory):
    lines = ['printf(" %%zu\\n", sizeof(%s));' % C_NAME] + ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f[0], C_NAME, f[0]) for f in Out._fields_]
    d = tmp_path_factory.mktemp("layout")
    src, exe = str(d / "layout.c"), str(d / "layout")
    open(src, "w").write('#include <stdio.h>\n#include "kshost.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(H.ROOT, "include"), src, "-o", exe])
    return {line.split(" ")[0]: int(line.split(" ")[1]) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()}


def test_the_struct_is_laid_out_as_the_header_says(header_layout):
    mine = {"": ctypes.sizeof(Out)}
    mine.update({f[0]: getattr(Out, f[0]).offset for f in Out._fields_})
    assert mine == header_layout, (mine, header_layout)
    assert sum(ctypes.sizeof(f[1]) for f in Out._fields_) == ctypes.sizeof(Out)      # no padding holes
    assert [f[0] for f in Out._fields_] == ["pod_flags", "cap_pods", "n_pods", "n_new", "n_placed", "n_unscheduled", "skipped_pods", "n_pods_flagged", "truncated", "used_classes",
                                            "checked", "pairs", "pad"]


# tests/test_audit_binding.py's child calls the claimed form with commit numbers for every pass but the first; this pass takes none
CHILD = TB.CHILD.replace('getattr(f, method)(res) if what == "audit" else getattr(f, method)(res, seq)', 'getattr(f, method)(res) if what in ("audit", "reasons") else getattr(f, method)(res, seq)')
EXPECTED = [["pod_flags", TB.P], ["n_pods_flagged", "int"], ["pod_bit_count", TB._by_name("REASON_PLACED", "REASON_MISSING", "REASON_SHAPE", "REASON_STATIC")],
            ["checked", TB._by_name("PODS", "EXACT", "BOUNDED", "UNEXAMINED")], ["skipped_pods", "int"], ["n_unscheduled", "int"], ["used_classes", "int"], ["pairs", "int"],
            ["n_new", "int"], ["n_placed", "int"], ["ms", TB.MS]]


@pytest.fixture(scope="module")
def returned():
    assert CHILD != TB.CHILD
    return H.run_emulated(CHILD, ["reasons"])


def test_the_dict_the_pass_returns_keeps_its_shape(returned):
    for form, got in zip(("resident", "claimed", "batch"), returned["reasons"]):
        assert got == EXPECTED, (form, got)


def test_the_other_tables_are_as_they_were():
    assert list(S._AUDIT_PASSES) == ["audit", "topology", "spread", "firstfit", "limits", "hostfit"] and list(S._AUDIT_PASSES_BESIDE) == ["stages"] and list(S._AUDIT_PASSES_REASONS) == ["reasons"]
    assert S.KS_AUDIT_PASS == {"audit": 1, "topology": 2, "spread": 4, "firstfit": 8, "limits": 16, "hostfit": 32}
    assert set(S._AUDIT_PASSES_REASONS["reasons"]) == set(S._AUDIT_PASSES["firstfit"])      # described in the same form
    assert S._AUDIT_PASSES_REASONS["reasons"]["claimed"] == (("pod_reason", "uint32"),) and not S._AUDIT_PASSES_REASONS["reasons"]["seq"]
    assert all("pod_reason" not in dict(p["claimed"]) for p in list(S._AUDIT_PASSES.values()) + list(S._AUDIT_PASSES_BESIDE.values()))      # for this pass only


def test_the_bits_and_reasons_are_the_headers():
    text = open(os.path.join(H.ROOT, "include", "ksolve.h")).read()
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define KS_AUDIT_POD_(REASON_\w+) (\d+)u", text)}
    assert bits == S.KS_AUDIT_REASONS_BITS and len(bits) == 4
    earlier = [int(m.group(1)) for m in re.finditer(r"#define KS_AUDIT_POD_(?!REASON_)\w+ (\d+)", text)]
    assert not set(earlier) & set(bits.values())      # a word of the pass's own would do; the bits are free all the same
    why = {m.group(1): int(m.group(2)) for m in re.finditer(r"KS_WHY_(\w+) = (\d+)", text)}
    assert why == S.KS_WHY
