"""(CPU) What the Python binding of the audit's ninth pass (karpenter_core_amd/scheduler.py _AUDIT_PASSES_ZONEFIT) must not move:
  a) the layout of the ctypes mirror of include/kshost.h's ksh_audit_zonefit_out, and of include/ksolve.h's ks_audit_zonefit as a second mirror written here, size
     and every member's offset against what a C99 compiler says of the headers;
  b) the bits and KS_AZ_GROUPS against the header;
  c) the fourth table leaves the three older tables, and with them the gate's mask bits, names and struct, as they were."""
import ctypes
import os
import subprocess

import pytest

import audit_harness as H
import audit_zonefit_ref as ZR
from karpenter_core_amd import scheduler as S

C_NAME, Out = "ksh_audit_zonefit_out", S._AuditZoneFitOut


class _Dev(ctypes.Structure):      # include/ksolve.h ks_audit_zonefit
    _fields_ = [("pod_flags", ctypes.c_void_p)] + [(n, ctypes.c_uint32) for n in ("n_pods", "n_new", "n_placed", "eligible_groups", "skipped_groups", "skipped_pods", "mixed_pods", "n_pods_flagged")] + \
               [("checked", ctypes.c_uint32 * 4), ("admitting_pairs", ctypes.c_uint32), ("exact_pods", ctypes.c_uint32), ("kernel_ms", ctypes.c_double), ("readback_ms", ctypes.c_double)]


@pytest.fixture(scope="module")
def header_layout(tmp_path_factory):
    lines = []
    for c_name, mirror in ((C_NAME, Out), ("ks_audit_zonefit", _Dev)):
        lines += ['printf("%s. %%zu\\n", sizeof(%s));' % (c_name, c_name)] + ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f[0], c_name, f[0]) for f in mirror._fields_]
    lines += ['printf("bits %u %u %u %u\\n", KS_AUDIT_POD_SEQ, KS_AUDIT_POD_ZFIT_EXISTING, KS_AUDIT_POD_ZFIT_NEW, KS_AZ_GROUPS);']
    d = tmp_path_factory.mktemp("layout")
    src, exe = str(d / "layout.c"), str(d / "layout")
    open(src, "w").write('#include <stddef.h>\n#include <stdio.h>\n#include "ksolve.h"\n#include "kshost.h"\nint main(void) {\n    %s\n    return 0;\n}\n' % "\n    ".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(H.ROOT, "include"), src, "-o", exe])
    return {line.split(" ")[0]: [int(x) for x in line.split(" ")[1:]] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()}


@pytest.mark.parametrize("c_name, mirror", [(C_NAME, Out), ("ks_audit_zonefit", _Dev)])
def test_the_struct_is_laid_out_as_the_header_says(header_layout, c_name, mirror):
    mine = {c_name + ".": [ctypes.sizeof(mirror)]}
    mine.update({c_name + "." + f[0]: [getattr(mirror, f[0]).offset] for f in mirror._fields_})
    assert mine == {k: v for k, v in header_layout.items() if k.startswith(c_name + ".")}, (mine, header_layout)
    assert sum(ctypes.sizeof(f[1]) for f in mirror._fields_) == ctypes.sizeof(mirror)      # no padding holes


def test_the_members_are_in_the_headers_order():
    assert [f[0] for f in Out._fields_] == ["pod_flags", "cap_pods", "n_pods", "n_new", "n_placed", "skipped_pods", "n_pods_flagged", "truncated", "eligible_groups", "skipped_groups", "mixed_pods",
                                            "exact_pods", "checked", "admitting_pairs", "pad"]


def test_the_bits_are_the_headers(header_layout):
    assert header_layout["bits"] == [S.KS_AUDIT_ZONEFIT_BITS["SEQ"], S.KS_AUDIT_ZONEFIT_BITS["ZFIT_EXISTING"], S.KS_AUDIT_ZONEFIT_BITS["ZFIT_NEW"], ZR.AZ_GROUPS]
    assert S.KS_AUDIT_ZONEFIT_BITS == ZR.BITS == {"SEQ": 128, "ZFIT_EXISTING": 67108864, "ZFIT_NEW": 134217728} and S.KS_AUDIT_ZONEFIT_CHECKED == ZR.CHECKED
    taken = 0
    for name in ("KS_AUDIT_POD_BITS", "KS_AUDIT_TOPOLOGY_BITS", "KS_AUDIT_SPREAD_BITS", "KS_AUDIT_FIRSTFIT_BITS", "KS_AUDIT_LIMITS_POD_BITS", "KS_AUDIT_HOSTFIT_BITS", "KS_AUDIT_STAGES_BITS", "KS_AUDIT_REASONS_BITS"):
        for v in getattr(S, name).values():
            taken |= v
    assert not taken & (67108864 | 134217728)      # the two new bits are no other pass's


def test_the_three_older_tables_and_the_gate_are_as_they_were():
    assert list(S._AUDIT_PASSES) == ["audit", "topology", "spread", "firstfit", "limits", "hostfit"] and list(S._AUDIT_PASSES_BESIDE) == ["stages"] and list(S._AUDIT_PASSES_REASONS) == ["reasons"]
    assert list(S._AUDIT_PASSES_ZONEFIT) == ["zonefit"] and set(S._AUDIT_PASSES_ZONEFIT["zonefit"]) == set(S._AUDIT_PASSES["hostfit"])      # described in the same form
    assert S.KS_AUDIT_PASS == {"audit": 1, "topology": 2, "spread": 4, "firstfit": 8, "limits": 16, "hostfit": 32}
    assert S.AUDIT_GATE_ALL == ("audit", "topology", "spread", "firstfit", "limits", "hostfit", "stages", "reasons") and list(S._AUDIT_PASSES_EX) == list(S.AUDIT_GATE_ALL)
    assert S.KS_AUDIT_PASS_EX == {name: 1 << i for i, name in enumerate(S.AUDIT_GATE_ALL)} and "zonefit" not in S.KS_AUDIT_PASS_EX
    assert callable(S.FlatProblem.audit_zonefit) and callable(S.audit_zonefit_batch)
