"""Which ks_pack instantiation a batch runs (karpenter_core_amd/csrc/ksolve.hip: pack_rows, pack_choose), through ks_debug_pack_choice / ks_debug_pack_row -- no
device needed.  Every combination of the chooser's eleven traits is compared with `chain_before_the_table`: a literal restatement of the if/else chains, the three
arrays of instantiations and the nested ternary that ks_solve_batch_dev held before the table existed (written from that code, not from the table).  The library
built by hipcc and the emulator build must both agree with it; each is loaded in a child process, so the pytest process keeps the libraries it has."""
import itertools
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

TRAITS = ("single", "fast", "bounds", "lean", "lean8", "wide", "one_wave", "tw128", "stats", "no_multi", "ladders44")      # bit i of the traits word (KS_PT_*)
KS_LEAN8_NW = 4
KS_RES_NARROW = 8

CHILD = r"""
import ctypes, json, sys
ks = ctypes.CDLL(sys.argv[1])
ks.ks_debug_pack_row.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
ks.ks_debug_pack_choice.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)]
f = (ctypes.c_int32 * 6)()
n = ks.ks_debug_pack_row(0xFFFFFFFF, f)
table = []
for i in range(n):
    assert ks.ks_debug_pack_row(i, f) == n
    table.append(list(f))
choices = []
for t in range(1 << 11):
    lds = ctypes.c_uint32(0)
    row = ks.ks_debug_pack_choice(t, f, ctypes.byref(lds))
    choices.append([row, list(f), lds.value])
json.dump({"table": table, "choices": choices}, sys.stdout)
"""


def chain_before_the_table(single, fast, bounds, lean, lean8, wide, one_wave, tw128, stats, no_multi, ladders44):
    """-> ((FAST, BOUNDS, LEAN, NW, RM), dynamic LDS bytes, pack_rm, pack_lean).  ks_pack<FAST, BOUNDS, LEAN, NW, RM = (LEAN ? 4 : KS_RES_NARROW)>."""
    def inst(f, b, l, nw, rm=None):
        return (int(f), int(b), int(l), nw, rm if rm is not None else (4 if l else KS_RES_NARROW))
    variants = [inst(False, False, False, 1), inst(False, True, False, 1), inst(True, False, False, 1), inst(True, True, False, 1),
                inst(False, False, True, 1), inst(False, True, True, 1), inst(True, False, True, 1), inst(True, True, True, 1)]
    variants_lean8 = [inst(False, False, True, 1, 8), inst(False, True, True, 1, 8), inst(True, False, True, 1, 8), inst(True, True, True, 1, 8)]
    variants_wide = [inst(False, False, False, 1, 16), inst(False, True, False, 1, 16), inst(True, False, False, 1, 16), inst(True, True, False, 1, 16)]
    lds_bytes = 100 * 1024 if single else 64 * 1024
    launched = None
    multi = single and fast and tw128 and not stats and not one_wave and not no_multi and not wide
    if multi:
        lds_mw = 44 * 1024
        if not ladders44:
            multi = False
        else:
            if lean and not bounds and lean8:
                launched = (inst(True, False, True, KS_LEAN8_NW, 8), lds_mw)
            elif lean and not bounds:
                launched = (inst(True, False, True, 8), lds_mw)
            elif bounds:
                launched = (inst(True, True, False, 4), lds_mw)
            else:
                launched = (inst(True, False, False, 4), lds_mw)
    if not multi and wide:
        launched = (variants_wide[(2 if fast else 0) + (1 if bounds else 0)], lds_bytes)
    elif not multi and lean and lean8:
        launched = (variants_lean8[(2 if fast else 0) + (1 if bounds else 0)], lds_bytes)
    elif not multi:
        launched = (variants[(4 if lean else 0) + (2 if fast else 0) + (1 if bounds else 0)], lds_bytes)
    pack_rm = 16 if wide else ((4 if lean and not bounds and not lean8 else KS_RES_NARROW) if multi else (4 if lean and not lean8 else KS_RES_NARROW))
    pack_lean = int(not wide and lean and not (multi and bounds))
    return launched[0], launched[1], pack_rm, pack_lean


def _library(which):
    if which == "hipcc":
        import __graft_entry__ as ge
        ge.build()
        return os.path.join(ROOT, "karpenter_core_amd", "libksolve.so")
    sys.path.insert(0, os.path.join(HERE, "sim"))
    import build_sim
    return os.path.join(build_sim.build(), "libksolve.so")


@pytest.mark.parametrize("which", ["hipcc", "emulator"])
def test_every_combination_of_traits_takes_the_instantiation_it_took_before(which):
    pr = subprocess.run([sys.executable, "-c", CHILD, _library(which)], capture_output=True, text=True, timeout=600)
    assert pr.returncode == 0, pr.stderr
    got = json.loads(pr.stdout)
    table = [tuple(r) for r in got["table"]]
    assert len(set(r[:5] for r in table)) == len(table), "an instantiation is listed twice"
    for r in table:      # the ceiling the attribute loop asks for: 104 KiB for a single-wave row, 44 KiB for a multi-wave one
        assert r[5] == (104 * 1024 if r[3] == 1 else 44 * 1024), r
    returned = set()
    assert len(got["choices"]) == 1 << len(TRAITS)
    for t, values in enumerate(itertools.product((False, True), repeat=len(TRAITS))):
        traits = dict(zip(reversed(TRAITS), values))      # (product counts like the traits word: the last factor is bit 0)
        assert sum(1 << i for i, k in enumerate(TRAITS) if traits[k]) == t
        row, fields, lds = got["choices"][t]
        want_inst, want_lds, want_rm, want_lean = chain_before_the_table(**traits)
        assert 0 <= row < len(table), (traits, row)
        assert tuple(fields) == table[row], (traits, row)
        assert tuple(fields[:5]) == want_inst, (traits, fields, want_inst)
        assert lds == want_lds and lds <= fields[5], (traits, lds, want_lds)
        assert (fields[4], fields[2]) == (want_rm, want_lean), (traits, fields, want_rm, want_lean)      # pack_rm, pack_lean: ks_solve_batch_dev stores the row's RM and LEAN
        returned.add(row)
    assert len(returned) == len(table), f"rows never chosen: {sorted(set(range(len(table))) - returned)}"
