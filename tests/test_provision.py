"""CPU: the Python mirror of the placement tables (karpenter_core_amd/scheduler.py decode_placement_head / decode_placement_row / placement_lists, provision /
placement_rows argument checks) against hand-made rows, and its layout constants against the headers.  The calls themselves: tests/test_provision_gpu.py."""
import os
import re

import numpy as np
import pytest

from karpenter_core_amd import scheduler as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(pod, where, stage, seq, reason, pid, position):
    u = lambda x: x & 0xFFFFFFFF
    return [u(pod) | (u(where) << 32), u(stage) | (u(seq) << 32), u(reason) | (u(pid) << 32), position]


def test_the_layout_constants_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "ksolve.h")).read() + open(os.path.join(ROOT, "include", "kshost.h")).read()
    for name in ("KS_PLC_HEAD_WORDS", "KS_PLC_ROW_WORDS", "KS_PLC_ID", "KS_PLC_P", "KS_PLC_N_NEW", "KS_PLC_N_UNSCHEDULED", "KS_PLC_ROW_OFF", "KS_PLC_FLAGS", "KS_PLC_N_EXISTING",
                 "KS_PLC_POD_WHERE", "KS_PLC_STAGE_SEQ", "KS_PLC_REASON_ID", "KS_PLC_POSITION", "KS_PLC_TRUNCATED", "KSH_PROVISION_MACHINES_TRUNCATED", "KSH_PROVISION_NOTHING",
                 "KSH_PROVISION_DERIVED", "KSH_PROVISION_FLATTENED"):
        m = re.search(r"#define %s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(S, name), name
    # the struct the mirror passes is the header's: the same members in the same order
    body = re.search(r"typedef struct ksh_provision_out \{(.*?)\} ksh_provision_out;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip().split()[-1].lstrip("*").split("[")[0] for decl in body.split(";") for m in decl.split(",") if m.strip()]
    assert members == [f[0] for f in S._ProvisionOut._fields_], members


def test_head_decoder():
    h = S.decode_placement_head([9, 14, 2, 1, 30, 0, 25, 0])
    assert h == {"id": 9, "pods": 14, "n_new": 2, "n_unscheduled": 1, "row_off": 30, "truncated": False, "machines_truncated": False, "n_existing": 25, "reserved": 0}
    assert S.decode_placement_head([0, 1, 0, 0, 0, S.KS_PLC_TRUNCATED, 3, 0])["truncated"] and not S.decode_placement_head([0, 1, 0, 0, 0, S.KS_PLC_TRUNCATED, 3, 0])["machines_truncated"]
    both = S.decode_placement_head(np.asarray([0, 1, 1, 0, 0, S.KS_PLC_TRUNCATED | S.KSH_PROVISION_MACHINES_TRUNCATED, 3, 0], dtype=np.uint64))
    assert both["truncated"] and both["machines_truncated"]


def test_row_decoder_signs_and_halves():
    E = 25
    d = S.decode_placement_row(_row(1234, 7, 0, 3, 0, 9, 0), E)
    assert d == {"pod": 1234, "where": 7, "existing": 7, "new": None, "stage": 0, "seq": 3, "reason": 0, "id": 9, "position": 0}
    d = S.decode_placement_row(_row(5, E + 2, 1, 0, 0, 0, 1), E)
    assert (d["existing"], d["new"], d["stage"]) == (None, 2, 1)
    d = S.decode_placement_row(_row(6, -1, 2, -1, 0x74, 0, 2), E)      # unscheduled: where and seq are -1 as int32, the reason word is kept whole
    assert (d["where"], d["existing"], d["new"], d["seq"], d["reason"], d["stage"]) == (-1, None, None, -1, 0x74, 2)
    d = S.decode_placement_row(np.asarray(_row(0xFFFFFFF0, E, 0, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 2 ** 40), dtype=np.uint64), E)
    assert (d["pod"], d["new"], d["seq"], d["reason"], d["id"], d["position"]) == (0xFFFFFFF0, 0, 0x7FFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 2 ** 40)
    assert S.decode_placement_row(_row(1, 0, 0, 0, 0, 0, 0), 0)["new"] == 0      # no existing node at all: slot 0 is new node 0


def test_lists_are_in_commit_order_not_row_order():
    E = 4
    rows = [S.decode_placement_row(r, E) for r in (_row(10, 4, 0, 5, 0, 0, 0), _row(11, 2, 0, 4, 0, 0, 1), _row(12, -1, 1, -1, 0x7, 0, 2), _row(13, 4, 2, 1, 0, 0, 3),
                                                   _row(14, 5, 0, 0, 0, 0, 4), _row(15, 2, 0, 2, 0, 0, 5), _row(16, -1, 0, -1, 0x4, 0, 6), _row(17, 4, 0, 3, 0, 0, 7))]
    ls = S.placement_lists(rows)
    assert ls["new"] == {0: [13, 17, 10], 1: [14]} and ls["existing"] == {2: [15, 11]}
    assert ls["unscheduled"] == [12, 16] and ls["reasons"] == {12: 0x7, 16: 0x4}      # queue order = row order
    assert ls["stage"] == {10: 0, 11: 0, 12: 1, 13: 2, 14: 0, 15: 0, 16: 0, 17: 0}
    assert S.placement_lists([]) == {"new": {}, "existing": {}, "unscheduled": [], "stage": {}, "reasons": {}}


def test_argument_checks_of_the_mirror():
    with pytest.raises(ValueError):
        S.placement_rows([], [1])                      # one id per handle
    with pytest.raises(ValueError):
        S.provision(None, [0], [0], 0)                 # a machine row needs at least one option word
    assert S.PROVISION_ROUTES == {0: "nothing", 1: "derived", 2: "flattened"}
