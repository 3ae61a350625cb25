"""The gate's reduction kernels apart from the passes (include/ksolve.h ks_audit_reduce_rows; karpenter_core_amd/csrc/ks_audit_reduce.inc ks_audit_tally,
ks_audit_tally_finish) against numpy, on the emulator (CPU) and, the same body, on the device (GPU).
Lengths: 0, 1, 63, 64, 65, 255, 256, 257 -- 257 is also one past where a table is cut into more than one workgroup's run --, 65 537 (64 runs, the most) and 16 385
(one past 64 whole tiles: the runs become longer than a tile).  Row contents: all zero, all 0xFFFFFFFF, one non-zero row at the first and at the last index, random
words at a density of 1 %.  Each with the four field shapes the passes' totals use: none (the first pass), topology's four, spread's three, first-fit's three."""
import numpy as np
import pytest

import audit_harness as H

LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 16385, 65537]
FIELDS = {"none": [], "topology": [(30, 3), (0, 1023), (10, 1023), (20, 1023)], "spread": [(30, 3), (0, 1023), (10, 1023)], "firstfit": [(30, 3), (0, 1), (29, 1)]}
CONTENTS = ["zero", "ones", "first", "last", "sparse"]


def rows_of(n, content, rng):
    r = np.zeros(n, dtype=np.uint32)
    if content == "ones":
        r[:] = 0xFFFFFFFF
    elif content == "first" and n:
        r[0] = rng.integers(1, 1 << 32)
    elif content == "last" and n:
        r[-1] = rng.integers(1, 1 << 32)
    elif content == "sparse" and n:
        at = np.nonzero(rng.random(n) < 0.01)[0]
        r[at] = rng.integers(1, 1 << 32, size=len(at), dtype=np.uint64).astype(np.uint32)
    return r


def expected(rows, fields):
    r = rows.astype(np.uint64)
    return {"n_set": int((rows != 0).sum()), "bit_count": [int(((r >> np.uint64(b)) & np.uint64(1)).sum()) for b in range(32)],
            "field_sum": [int(((r >> np.uint64(s)) & np.uint64(m)).sum() % (1 << 32)) for s, m in fields]}


def body(S):
    """Every (length, content, field shape) through S.audit_reduce_rows against numpy; returns the cases that differ."""
    rng, bad, n_cases = np.random.default_rng(33), [], 0
    for n in LENGTHS:
        for content in CONTENTS:
            rows = rows_of(n, content, rng)
            for shape, fields in FIELDS.items():
                got, want = S.audit_reduce_rows(rows, fields), expected(rows, fields)
                n_cases += 1
                if got != want:
                    bad.append([n, content, shape, str({k: (got[k], want[k]) for k in want if got[k] != want[k]})[:300]])
    return {"cases": n_cases, "bad": bad}


CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import simlib
S = simlib.use_sim()
import test_audit_reduce_rows as T
print("RESULT " + json.dumps(T.body(S)))
"""


def _check(got):
    assert got["cases"] == len(LENGTHS) * len(CONTENTS) * len(FIELDS)
    assert not got["bad"], got["bad"][:5]


def test_reduce_rows_against_numpy_on_the_emulator():
    _check(H.run_emulated(CHILD))


@pytest.mark.gpu
def test_reduce_rows_against_numpy_on_the_device():
    from karpenter_core_amd import scheduler as S
    _check(body(S))


def test_the_expectation_itself_on_a_hand_made_table():
    rows = np.array([0, 1, 0x80000001, 0xC0000400], dtype=np.uint32)
    assert expected(rows, FIELDS["topology"]) == {"n_set": 3, "bit_count": [2] + [0] * 9 + [1] + [0] * 19 + [1, 2], "field_sum": [2 + 3, 1 + 1 + 0, 1, 0]}
