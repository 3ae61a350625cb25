"""(CPU) What the Python binding of the audit's seventh pass (karpenter_core_amd/scheduler.py _AUDIT_PASSES_BESIDE) must not move -- tests/test_audit_binding.py's
method for the new struct only:
  a) the layout of the ctypes mirror of include/kshost.h's ksh_audit_stages_out, size and every member's offset against what a C99 compiler says of the header;
  b) the shape of the dict the pass returns in resident, claimed and batch form, over the smallest problem with a new node and an unscheduled pod, on the emulator;
  c) the table beside _AUDIT_PASSES leaves that table, and with it the gate's mask bits and struct, as they were."""
import ctypes
import os
import subprocess

import pytest

import audit_harness as H
import test_audit_binding as TB
from karpenter_core_amd import scheduler as S

C_NAME, Out = "ksh_audit_stages_out", S._AuditStagesOut


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
    assert [f[0] for f in Out._fields_] == ["pod_flags", "cap_pods", "n_pods", "n_new", "n_placed", "skipped_pods", "n_pods_flagged", "truncated", "checked", "admitting_pairs", "pad"]


EXPECTED = [["pod_flags", TB.P], ["n_pods_flagged", "int"], ["pod_bit_count", TB._by_name("SEQ", "STAGE_EXISTING", "STAGE_TEMPLATE", "STAGE_UNRELAXED")],
            ["checked", TB._by_name("SEQ", "PODS", "STAGES", "PAIRS")], ["admitting_pairs", "int"], ["skipped_pods", "int"], ["n_new", "int"], ["n_placed", "int"], ["ms", TB.MS]]


@pytest.fixture(scope="module")
def returned():
    return H.run_emulated(TB.CHILD, ["stages"])


def test_the_dict_the_pass_returns_has_the_fourth_passes_shape(returned):
    for form, got in zip(("resident", "claimed", "batch"), returned["stages"]):
        assert got == EXPECTED, (form, got)


def test_the_gates_table_is_as_it_was():
    assert list(S._AUDIT_PASSES) == ["audit", "topology", "spread", "firstfit", "limits", "hostfit"] and list(S._AUDIT_PASSES_BESIDE) == ["stages"]
    assert S.KS_AUDIT_PASS == {"audit": 1, "topology": 2, "spread": 4, "firstfit": 8, "limits": 16, "hostfit": 32}
    assert set(S._AUDIT_PASSES_BESIDE["stages"]) == set(S._AUDIT_PASSES["firstfit"])      # described in the same form
    assert S.KS_AUDIT_STAGES_BITS == {"SEQ": 128, "STAGE_EXISTING": 524288, "STAGE_TEMPLATE": 1048576, "STAGE_UNRELAXED": 2097152}
