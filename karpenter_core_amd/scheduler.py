"""Host-side mirror of the reference scheduler interface for the hot path, over the C ABI.

Reference call sites this stands in for (paths relative to aws/karpenter-core pkg/):

    scheduler, err := p.NewScheduler(ctx, pods, stateNodes, opts)     controllers/provisioning/provisioner.go:301
    nodes, existing, err := scheduler.Solve(ctx, pods)                 provisioner.go:307, deprovisioning/helpers.go:93

`NewScheduler(...)` assembles the semantic problem (provisioners -> machine templates, instance types,
state nodes, cluster pods for topology counting, daemonset pods) and hands it to libkshost.so, which
runs the host half (NewTopology / flattening, host/encode.cpp) and calls libksolve.so's HIP kernels
through the C ABI (include/ksolve.h).  `Scheduler.Solve(pods)` returns `(new_nodes, existing_nodes,
None)` -- the error is always None, exactly like scheduler.go:132.

There is NO CPU scheduling path: if the HIP library is missing, or no gfx950 device is visible, every
call raises.  (The CPU oracle lives in oracle/ and is test infrastructure only.)
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from .model import (ClusterPod, InstanceType, NewNodeOut, Pod, Problem, Provisioner, SolveResult, StateNode,
                    parse_result)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBS = None

KS_OK, KS_ERR_INVALID, KS_ERR_UNSUPPORTED, KS_ERR_DEVICE, KS_ERR_CAPACITY = 0, -1, -2, -3, -4
KS_FLAG_SIMULATION, KS_FLAG_STATS, KS_FLAG_NO_RR, KS_FLAG_ONE_WAVE, KS_FLAG_NO_LEAN = 1, 2, 4, 8, 16
KSH_DERIVE_VOLUMES = 1 << 16      # kshost.h: derive what-ifs over snapshots with CSI volume limits / claims too (opt-in)
KSH_DERIVE_GROUP_LISTS = 1 << 18  # kshost.h: hold a derived what-if's per-node topology facts as lists per node -- any number of topology groups (opt-in)
KSH_ACTIVE_RESOURCES = 1 << 17    # kshost.h: flatten over the resource names the problem requests or limits, not over all a catalogue lists (opt-in)
KSH_APPLY_TRACK_CLUSTER_PODS = 1  # kshost.h: ksh_env_apply_block mirrors BIND / UNBIND into the cluster pods whatever the snapshot started with
# ksolve.h KS_AUDIT_*: the bits of FlatProblem.audit() / audit_batch(), by name
KS_AUDIT_POD_BITS = {"RANGE": 1, "UNSCHEDULED_LIST": 2, "TAINTS": 4, "REQUIREMENTS": 8, "HOSTNAME": 16, "PORTS": 32, "VOLUME_ERROR": 64}
KS_AUDIT_NODE_BITS = {"RESOURCES": 1, "VOLUMES": 2, "EMPTY": 4, "TEMPLATE": 8, "REQUESTS": 16, "OPTIONS_EMPTY": 32, "OPTIONS_EXTRA": 64, "OPTIONS_MISSING": 128}
KSH_AUDIT_TRUNCATED_PODS, KSH_AUDIT_TRUNCATED_NODES = 1, 2
# the second pass's bits (FlatProblem.audit_topology() / audit_topology_batch()), a word of their own, and what `checked` counts per rule
KS_AUDIT_TOPOLOGY_BITS = {"SEQ": 128, "ANTI_AFFINITY": 256, "AFFINITY": 512, "HOSTNAME_SPREAD": 1024}
KS_AUDIT_TOPOLOGY_RULES = ("SEQ", "ANTI_AFFINITY", "AFFINITY", "HOSTNAME_SPREAD")
# the third pass's (FlatProblem.audit_spread() / audit_spread_batch()): SEQ as above, and spread over narrow keys
KS_AUDIT_SPREAD_BITS = {"SEQ": 128, "SPREAD": 2048}
KS_AUDIT_SPREAD_RULES = ("SEQ", "SPREAD")
# the fourth pass's (FlatProblem.audit_firstfit() / audit_firstfit_batch()): SEQ as above, and first-fit order; `checked`: placed pods, examined pods, (class, node) pairs
KS_AUDIT_FIRSTFIT_BITS = {"SEQ": 128, "FIT_EXISTING": 4096, "FIT_NEW": 8192, "FIT_TEMPLATE": 16384}
KS_AUDIT_FIRSTFIT_CHECKED = ("SEQ", "PODS", "PAIRS")
# the fifth pass's (FlatProblem.audit_limits() / audit_limits_batch()): SEQ as above, and provisioner limits in opening order; its node bits continue KS_AUDIT_NODE_BITS
# in a word of the pass's own; `checked`: placed pods, new nodes of limited templates, examined pods, (class, template) pairs
KS_AUDIT_LIMITS_POD_BITS = {"SEQ": 128, "LIMIT_TEMPLATE": 32768}
KS_AUDIT_LIMITS_NODE_BITS = {"LIMIT_EXTRA": 256, "LIMIT_MISSING": 512}
KS_AUDIT_LIMITS_CHECKED = ("SEQ", "NODES", "PODS", "PAIRS")
# the sixth pass's (FlatProblem.audit_hostfit() / audit_hostfit_batch()): SEQ as above, and first-fit order for pods under hostname anti-affinity / hostname spread;
# `checked`: placed pods, examined pods, (class, node) pairs, (pair, group) count tests
KS_AUDIT_HOSTFIT_BITS = {"SEQ": 128, "HFIT_EXISTING": 65536, "HFIT_NEW": 131072, "HFIT_TEMPLATE": 262144}
KS_AUDIT_HOSTFIT_CHECKED = ("SEQ", "PODS", "PAIRS", "TESTS")
# the seventh pass's (FlatProblem.audit_stages() / audit_stages_batch()): SEQ as above, and relaxation order -- a pod's earlier stages against the existing nodes' final
# state and fresh machines of unlimited templates; `checked`: placed pods, pods with an examined stage, examined stages, (class, node-or-template) pairs
KS_AUDIT_STAGES_BITS = {"SEQ": 128, "STAGE_EXISTING": 524288, "STAGE_TEMPLATE": 1048576, "STAGE_UNRELAXED": 2097152}
KS_AUDIT_STAGES_CHECKED = ("SEQ", "PODS", "STAGES", "PAIRS")
# the eighth pass's (FlatProblem.audit_reasons() / audit_reasons_batch()): pod_reason's nibbles (KS_WHY_* per machine template) against what a fresh node of every template
# answers the pod's class; `checked`: unscheduled pods examined, nibbles decided exactly, nibbles bounded to a set, nibbles not examined
KS_AUDIT_REASONS_BITS = {"REASON_PLACED": 4194304, "REASON_MISSING": 8388608, "REASON_SHAPE": 16777216, "REASON_STATIC": 33554432}
KS_AUDIT_REASONS_CHECKED = ("PODS", "EXACT", "BOUNDED", "UNEXAMINED")
# the ninth pass's (FlatProblem.audit_zonefit() / audit_zonefit_batch()), beside the gate: SEQ as above, and first-fit order for pods under zonal spread; `checked`: placed
# pods, examined pods, (pod, node) pairs whose zone test ran, pairs that passed it
KS_AUDIT_ZONEFIT_BITS = {"SEQ": 128, "ZFIT_EXISTING": 67108864, "ZFIT_NEW": 134217728}
KS_AUDIT_ZONEFIT_CHECKED = ("SEQ", "PODS", "ZONE", "STATIC")
KS_WHY = {"NONE": 0, "LIMITS": 1, "TAINTS": 2, "HOST_PORTS": 3, "REQUIREMENTS": 4, "TOPOLOGY": 5, "TOPOLOGY_REQS": 6, "NO_INSTANCE_TYPE": 7}      # ksolve.h KS_WHY_*


class KSolveError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ksolve error {code}: {msg}")
        self.code = code


def libs():
    """Load libksolve.so (HIP kernels + C ABI) and libkshost.so (host side).  Fails loudly."""
    global _LIBS
    if _LIBS is None:
        ks_path = os.path.join(_HERE, "libksolve.so")
        kh_path = os.path.join(_HERE, "libkshost.so")
        for p in (ks_path, kh_path):
            if not os.path.exists(p):
                raise KSolveError(KS_ERR_DEVICE, f"{p} is missing -- build it with __graft_entry__.build(); "
                                                 "there is no Python/CPU fallback for the scheduling path")
        ks = ctypes.CDLL(ks_path, mode=ctypes.RTLD_GLOBAL)
        kh = ctypes.CDLL(kh_path)
        ks.ks_device_count.restype = ctypes.c_int
        ks.ks_last_error.restype = ctypes.c_char_p
        ks.ks_version.restype = ctypes.c_char_p
        kh.ksh_last_error.restype = ctypes.c_char_p
        kh.ksh_open.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
        kh.ksh_close.argtypes = [ctypes.c_void_p]
        kh.ksh_upload.argtypes = [ctypes.c_void_p, ctypes.c_int]
        kh.ksh_upload_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]
        kh.ksh_result_summaries.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
        kh.ksh_solve.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_solve_batch.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_grid.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        kh.ksh_grid_rows.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        kh.ksh_grid_install.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
        kh.ksh_debug_grid.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        kh.ksh_debug_pod_classes.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        kh.ksh_debug_whatif_topology.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        kh.ksh_whatifs_arena_bytes.argtypes = [ctypes.c_void_p]
        kh.ksh_whatifs_arena_bytes.restype = ctypes.c_uint64
        kh.ksh_whatifs_upload_bytes.argtypes = [ctypes.c_void_p]
        kh.ksh_whatifs_upload_bytes.restype = ctypes.c_uint64
        kh.ksh_debug_classes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        kh.ksh_price_filter.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32),
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        kh.ksh_dims.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        kh.ksh_rr_status.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        kh.ksh_pack_width.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        kh.ksh_pack_lean.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        kh.ksh_pack_row.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        ks.ks_debug_pack_row.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
        kh.ksh_solve_whatifs_sharded.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        ks.ks_deal_lpt.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        ks.ks_deal_lpt.restype = None
        kh.ksh_result_arrays_get.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        kh.ksh_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        kh.ksh_name.restype = ctypes.c_char_p
        kh.ksh_open_whatifs.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                        ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
        kh.ksh_parse.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
        kh.ksh_parsed_free.argtypes = [ctypes.c_void_p]
        kh.ksh_solve_from_pods.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_result_text.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        kh.ksh_result_summary.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        kh.ksh_open_whatifs_parsed.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                               ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
        kh.ksh_launch_pick.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_key_value.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int32]
        kh.ksh_key_value.restype = ctypes.c_char_p
        kh.ksh_types_subset.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32,
                                        ctypes.POINTER(ctypes.c_uint32)]
        kh.ksh_solve_batch_resident.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_result_records_dev.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.c_void_p]
        kh.ksh_fingerprint.argtypes = [ctypes.c_void_p]
        kh.ksh_fingerprint.restype = ctypes.c_uint64
        kh.ksh_free.argtypes = [ctypes.c_void_p]
        kh.ksh_open_whatifs_derived.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                                ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        kh.ksh_pods_ingest.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_env_ingest.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_pods_free.argtypes = [ctypes.c_void_p]
        kh.ksh_pods_count.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        kh.ksh_solve_from_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_double)]
        kh.ksh_open_batch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
        _LIBS = (ks, kh)
    return _LIBS


def device_count() -> int:
    return int(libs()[0].ks_device_count())


# ---- mirrors of the per-class device records (csrc/ksolve.hip), read back by FlatProblem.class_tables() ----
KS_RES_NARROW, KS_MAX_TOUCH, KS_MAX_TOPO, KS_MAX_HOST, KS_MAX_REC = 8, 12, 24, 3, 24


class PlanTouch(ctypes.Structure):
    _fields_ = [("mask", ctypes.c_uint64), ("gt", ctypes.c_int32), ("lt", ctypes.c_int32), ("key", ctypes.c_int32), ("own", ctypes.c_uint8), ("complement", ctypes.c_uint8),
                ("topo_begin", ctypes.c_uint8), ("topo_end", ctypes.c_uint8)]


class PlanTopo(ctypes.Structure):
    _fields_ = [("PD", ctypes.c_uint64), ("g", ctypes.c_int32), ("maxskew", ctypes.c_int32), ("type", ctypes.c_uint8), ("self", ctypes.c_uint8), ("pod_has", ctypes.c_uint8),
                ("hslot", ctypes.c_uint8), ("hrow", ctypes.c_uint32)]


class PlanRec(ctypes.Structure):
    _fields_ = [("g", ctypes.c_int32), ("key", ctypes.c_int32), ("type", ctypes.c_uint8), ("owned_inverse", ctypes.c_uint8), ("hslot", ctypes.c_uint16), ("tidx", ctypes.c_uint8),
                ("filtered", ctypes.c_uint8), ("pad", ctypes.c_uint16)]


class ClsPlan(ctypes.Structure):      # alignas(16): the tail pads the record to the next multiple of 16 bytes
    _fields_ = [("c", ctypes.c_uint32), ("present", ctypes.c_uint32), ("complement", ctypes.c_uint32), ("it_state", ctypes.c_int32),
                ("hn_mode", ctypes.c_uint32), ("hn_off", ctypes.c_uint32), ("hn_cnt", ctypes.c_uint32), ("reqmask", ctypes.c_uint32),
                ("tol", ctypes.c_uint64), ("port_off", ctypes.c_uint32), ("port_cnt", ctypes.c_uint32),
                ("vol_off", ctypes.c_uint32), ("vol_cnt", ctypes.c_uint32), ("mono", ctypes.c_uint32), ("dyn", ctypes.c_uint32),
                ("ntouch", ctypes.c_uint32), ("ntopo", ctypes.c_uint32), ("nhost", ctypes.c_uint32), ("nrec", ctypes.c_uint32),
                ("req", ctypes.c_int64 * KS_RES_NARROW), ("touch", PlanTouch * KS_MAX_TOUCH), ("topo", PlanTopo * KS_MAX_TOPO), ("host", PlanTopo * KS_MAX_HOST),
                ("rec", PlanRec * KS_MAX_REC), ("tmask", ctypes.c_uint64), ("rmask", ctypes.c_uint64), ("overflow", ctypes.c_uint32), ("eq", ctypes.c_uint32),
                ("tkeys", ctypes.c_uint64), ("_tail", ctypes.c_uint8 * 8)]


class ClsBrief(ctypes.Structure):
    _fields_ = [("tmask", ctypes.c_uint64), ("tfull", ctypes.c_uint64), ("rmask", ctypes.c_uint64), ("ev", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reqmask", ctypes.c_uint32), ("dyn", ctypes.c_uint32), ("req", ctypes.c_int64 * KS_RES_NARROW), ("zmask", ctypes.c_uint64), ("rsure", ctypes.c_uint64),
                ("dyn_maxskew", ctypes.c_int32), ("dyn_pd", ctypes.c_uint32)]


class _ProblemHead(ctypes.Structure):      # include/ksolve.h ks_problem, up to the offering arrays (FlatProblem.catalogue)
    _fields_ = [(n, ctypes.c_uint32) for n in ("P", "C", "T", "M", "E", "K", "R", "G", "GH", "S", "SC", "max_new_nodes", "flags", "wellknown_mask")] + [
        ("key_nvalues", ctypes.POINTER(ctypes.c_uint32)), ("value_int", ctypes.POINTER(ctypes.c_int32)), ("key_zone", ctypes.c_int32), ("key_ct", ctypes.c_int32),
        ("n_ct", ctypes.c_uint32), ("it_present", ctypes.POINTER(ctypes.c_uint32)), ("it_complement", ctypes.POINTER(ctypes.c_uint32)),
        ("it_mask", ctypes.POINTER(ctypes.c_uint64)), ("it_alloc", ctypes.POINTER(ctypes.c_int64)), ("it_cap", ctypes.POINTER(ctypes.c_int64)),
        ("it_offer", ctypes.POINTER(ctypes.c_uint64)), ("it_price", ctypes.POINTER(ctypes.c_double)), ("it_price_lo", ctypes.POINTER(ctypes.c_double))]


class FlatProblem:
    """A Solve() problem flattened to the C-ABI `ks_problem` (host side only until `upload`)."""

    def __init__(self, problem: Optional[Problem], stats: bool = False, _handle=None, flags: int = 0, active_resources: bool = False):
        ks, kh = libs()
        if _handle is not None:
            self._h = _handle
        else:
            text = problem.to_ksp().encode()
            self._h = ctypes.c_void_p()
            flags = (KS_FLAG_STATS if stats else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags      # (KS_FLAG_NO_RR / _ONE_WAVE / _NO_LEAN: the kernel choice travels with the problem)
            rc = kh.ksh_open(text, len(text), flags, ctypes.byref(self._h))
            if rc != KS_OK:
                raise KSolveError(rc, kh.ksh_last_error().decode())
        d = (ctypes.c_uint32 * 10)()
        kh.ksh_dims(self._h, d)
        self.dims = dict(zip(["P", "C", "T", "M", "E", "K", "R", "G", "GH", "S"], [int(x) for x in d]))
        self.kernel_ms = None
        self.wall_ms = None

    def fingerprint(self) -> int:
        """Hash of every array of the flat problem (equal iff two construction routes flattened to the same ks_problem)."""
        return int(libs()[1].ksh_fingerprint(self._h))

    def close(self):
        if self._h:
            libs()[1].ksh_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, device: int = 0):
        rc = libs()[1].ksh_upload(self._h, device)
        if rc != KS_OK:
            raise KSolveError(rc, libs()[1].ksh_last_error().decode())

    def solve(self, decode: bool = True) -> Optional[SolveResult]:
        ks, kh = libs()
        out = ctypes.c_void_p()
        kms, wms = ctypes.c_float(), ctypes.c_double()
        rc = kh.ksh_solve(self._h, ctypes.byref(out) if decode else None, ctypes.byref(kms), ctypes.byref(wms))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        self.kernel_ms, self.wall_ms = float(kms.value), float(wms.value)
        if not decode:
            return None
        text = ctypes.string_at(out).decode()
        kh.ksh_free(out)
        return parse_result(text)

    def rr_status(self):
        """(ks_pack_rr was launched for the last solve, why it declined -- 0: it took the Solve; codes in csrc/ks_pack_rr.inc).  include/ksolve.h ks_problem_rr_status."""
        out = (ctypes.c_int * 2)()
        rc = libs()[1].ksh_rr_status(self._h, out)
        if rc != KS_OK:
            raise KSolveError(rc, "ksh_rr_status")
        return bool(out[0]), int(out[1])

    def pack_width(self) -> int:
        """Resource bound of the ks_pack variant that took the last solve: 4 (LEAN), 8, 16 (a problem with more than 8 resource names); 0 if ks_pack_rr took it.
        include/ksolve.h ks_problem_pack_width."""
        out = ctypes.c_int()
        rc = libs()[1].ksh_pack_width(self._h, ctypes.byref(out))
        if rc != KS_OK:
            raise KSolveError(rc, "ksh_pack_width")
        return int(out.value)

    def pack_lean(self) -> bool:
        """Whether the ks_pack variant that took the last solve was a LEAN one (width 4, or 8 for a problem flattened with `active_resources`); False if ks_pack_rr
        took it.  include/ksolve.h ks_problem_pack_lean."""
        out = ctypes.c_int()
        rc = libs()[1].ksh_pack_lean(self._h, ctypes.byref(out))
        if rc != KS_OK:
            raise KSolveError(rc, "ksh_pack_lean")
        return bool(out.value)

    def pack_row(self):
        """Which ks_pack instantiation took the last solve (alone or as a member of a batch): (row, FAST, BOUNDS, LEAN, NW, RM) -- the row's index in the library's
        table and its fields as `ks_debug_pack_row` names them -- or None if ks_pack_rr took it or nothing ran.  include/ksolve.h ks_problem_pack_row."""
        ks, kh = libs()
        out = ctypes.c_int()
        rc = kh.ksh_pack_row(self._h, ctypes.byref(out))
        if rc != KS_OK:
            raise KSolveError(rc, "ksh_pack_row")
        row = int(out.value)
        if row < 0:
            return None
        f = (ctypes.c_int32 * 6)()
        if row >= ks.ks_debug_pack_row(row, f):
            raise KSolveError(KS_ERR_INVALID, f"ksh_pack_row: row {row} is not in the table")
        return (row, bool(f[0]), bool(f[1]), bool(f[2]), int(f[3]), int(f[4]))

    def catalogue(self) -> dict:
        """The offering arrays of the flat problem as `ksh_problem` shows them (include/ksolve.h ks_problem): {"it_offer": [T] available (zone, capacity-type)
        pairs, "it_price" / "it_price_lo": [T, NP] highest / lowest price of an available pair, -1 / DBL_MAX where there is none}.  Copies."""
        import numpy as np
        kh = libs()[1]
        kh.ksh_problem.restype = ctypes.POINTER(_ProblemHead)
        kh.ksh_problem.argtypes = [ctypes.c_void_p]
        p = kh.ksh_problem(self._h).contents
        t = int(p.T)
        npairs = int(p.key_nvalues[p.key_zone]) * int(p.n_ct)
        out = {"it_offer": np.ctypeslib.as_array(p.it_offer, shape=(t,)).copy() if t else np.zeros(0, dtype=np.uint64)}
        for k, ptr in (("it_price", p.it_price), ("it_price_lo", p.it_price_lo)):
            out[k] = np.ctypeslib.as_array(ptr, shape=(t, npairs)).copy() if t and npairs and ptr else np.zeros((t, npairs))
        return out

    def resource_names(self) -> List[str]:
        """The resource universe of the flat problem, by id (kshost.h ksh_name(h, 2, r, 0)): with `active_resources` the active names only."""
        kh = libs()[1]
        return [kh.ksh_name(self._h, 2, r, 0).decode() for r in range(self.dims["R"])]

    def result_arrays(self) -> dict:
        """The result through the binary door (include/kshost.h ksh_result_arrays_get): numpy copies of the arrays plus the key / resource names."""
        import numpy as np

        class RA(ctypes.Structure):
            _fields_ = [(n, ctypes.c_uint32) for n in ("n_pods", "n_existing", "n_new", "n_unscheduled", "types_words", "n_resources", "n_keys", "pad")] + \
                       [(n, ctypes.c_void_p) for n in ("pod_node", "pod_stage", "pod_reason", "unscheduled", "node_pods_off", "node_pods", "node_tmpl", "node_types", "node_requests",
                                                       "node_requests_present", "node_present", "node_complement", "node_mask", "node_gt", "node_lt", "node_it_state")]
        kh = libs()[1]
        ra = RA()
        rc = kh.ksh_result_arrays_get(self._h, ctypes.byref(ra))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())

        def arr(ptr, n, dt):
            if not n or not ptr:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(n,)).copy()
        P, E, N, K, R, TW = ra.n_pods, ra.n_existing, ra.n_new, ra.n_keys, ra.n_resources, ra.types_words
        off = arr(ra.node_pods_off, E + N + 1, np.uint32)
        return {"n_existing": E, "n_new": N, "pod_node": arr(ra.pod_node, P, np.int32), "pod_stage": arr(ra.pod_stage, P, np.int32), "pod_reason": arr(ra.pod_reason, P, np.uint32),
                "unscheduled": arr(ra.unscheduled, ra.n_unscheduled, np.int32), "node_pods_off": off, "node_pods": arr(ra.node_pods, int(off[-1]) if len(off) else 0, np.int32),
                "node_tmpl": arr(ra.node_tmpl, N, np.int32), "node_types": arr(ra.node_types, N * TW, np.uint64).reshape(N, TW), "node_requests": arr(ra.node_requests, N * R, np.int64).reshape(N, R),
                "node_requests_present": arr(ra.node_requests_present, N, np.uint32), "node_present": arr(ra.node_present, N, np.uint32), "node_complement": arr(ra.node_complement, N, np.uint32),
                "node_mask": arr(ra.node_mask, N * K, np.uint64).reshape(N, K), "node_gt": arr(ra.node_gt, N * K, np.int32).reshape(N, K), "node_lt": arr(ra.node_lt, N * K, np.int32).reshape(N, K),
                "node_it_state": arr(ra.node_it_state, N, np.int32),
                "key_names": [(kh.ksh_name(self._h, 0, k, 0) or b"").decode() for k in range(K)], "resource_names": [(kh.ksh_name(self._h, 2, r, 0) or b"").decode() for r in range(R)],
                "key_value": lambda k, v: (kh.ksh_name(self._h, 1, k, v) or b"").decode()}

    def audit(self, claimed: Optional[dict] = None) -> dict:
        """Audit a result against this problem on the device (include/ksolve.h KS_AUDIT_*, kshost.h ksh_audit / ksh_audit_claimed).  Without `claimed`: the result the
        last solve left on the device.  With `claimed`: a result in `result_arrays()`' form -- from anywhere -- is uploaded and audited instead (flattened problems
        only).  Returns {"pod_flags": uint32 [P], "node_flags": uint32 [E + n_new], "n_pods_flagged", "n_nodes_flagged", "pod_bit_count", "node_bit_count" (by bit
        name), "n_new", "n_unscheduled", "ms": (kernels, read-back)}; a clean result has no flag set."""
        return _audit("audit", [self], claimed)[0]

    def pod_seq(self):
        """The commit numbers of the result on the device, int32 [P] by pod index (-1: unscheduled), read through `ksh_placement_rows` (KS_PLC_STAGE_SEQ).  For a
        Solve's handle: the rows of a what-if over a snapshot name the snapshot's pods, not the what-if's own (`placement_rows`)."""
        import numpy as np
        heads, rows, _ = placement_rows([self], [0])
        seq = np.full(int(heads[0][KS_PLC_P]), -1, dtype=np.int32)
        if rows is not None and len(seq):
            seq[(rows[:, KS_PLC_POD_WHERE] & np.uint64(0xFFFFFFFF)).astype(np.int64)] = (rows[:, KS_PLC_STAGE_SEQ] >> np.uint64(32)).astype(np.uint32).view(np.int32)
        return seq

    def audit_topology(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's second, opt-in pass (include/ksolve.h KS_AUDIT_POD_SEQ .., kshost.h ksh_audit_topology / ksh_audit_topology_claimed): pod (anti-)affinity and hostname
        spread, decided from the final state and the commit numbers.  Without `claimed`: the result on the device.  With `claimed` (a result in `result_arrays()`' form)
        and `pod_seq` (int32 [P], as `pod_seq()` returns it): those are uploaded and audited instead (flattened problems only).  Returns {"pod_flags": uint32 [P],
        "n_pods_flagged", "pod_bit_count" and "checked" (by rule name), "skipped_groups", "n_new", "n_placed", "ms"}."""
        return _audit("topology", [self], claimed, pod_seq)[0]

    def audit_spread(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's third, opt-in pass (include/ksolve.h KS_AUDIT_POD_SPREAD, kshost.h ksh_audit_spread / ksh_audit_spread_claimed): topology spread over narrow keys --
        the zone --, decided from the final state and the commit numbers.  Arguments as `audit_topology`'s.  Returns {"pod_flags": uint32 [P], "n_pods_flagged",
        "pod_bit_count" and "checked" (by rule name: SEQ the placed pods, SPREAD the (pod, group) pairs examined), "exact_pairs", "skipped_groups", "n_new", "n_placed", "ms"}."""
        return _audit("spread", [self], claimed, pod_seq)[0]

    def audit_firstfit(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's fourth, opt-in pass (include/ksolve.h KS_AUDIT_POD_FIT_*, kshost.h ksh_audit_firstfit / ksh_audit_firstfit_claimed): first-fit order -- no pod ended
        later than an existing node, a new node or a template whose final state would still take it --, decided from the final state and the commit numbers.  Arguments
        as `audit_topology`'s.  Returns {"pod_flags": uint32 [P], "n_pods_flagged", "pod_bit_count", "checked" (SEQ the placed pods, PODS the pods examined, PAIRS the
        (class, node-or-template) pairs evaluated), "admitting_pairs", "skipped_pods", "n_new", "n_placed", "ms"}."""
        return _audit("firstfit", [self], claimed, pod_seq)[0]

    def audit_limits(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's fifth, opt-in pass (include/ksolve.h KS_AUDIT_NODE_LIMIT_*, KS_AUDIT_POD_LIMIT_TEMPLATE, kshost.h ksh_audit_limits / ksh_audit_limits_claimed):
        provisioner limits -- no machine of a limited provisioner holds a type above what can have remained when it opened or lacks one that must have remained, no pod
        passed over a limited provisioner that still had room --, decided from the final state and the commit numbers.  Arguments as `audit_topology`'s.  Returns
        `audit_firstfit`'s dict ("checked": SEQ the placed pods, NODES the new nodes of limited templates, PODS the pods examined, PAIRS the (class, template) pairs)
        plus "node_flags" (uint32 [E + n_new]), "n_nodes_flagged", "node_bit_count", "limited_templates", "exact_nodes", "binding_nodes" and "skipped_nodes"."""
        return _audit("limits", [self], claimed, pod_seq)[0]

    def audit_hostfit(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's sixth, opt-in pass (include/ksolve.h KS_AUDIT_POD_HFIT_*, kshost.h ksh_audit_hostfit / ksh_audit_hostfit_claimed): the fourth pass's first-fit order
        for the pods whose constraining groups are all hostname anti-affinity or unfiltered hostname spread.  Arguments as `audit_topology`'s.  Returns
        `audit_firstfit`'s dict ("checked": SEQ, PODS, PAIRS and TESTS, the (pair, group) count tests evaluated) plus "eligible_groups" and "skipped_groups"."""
        return _audit("hostfit", [self], claimed, pod_seq)[0]

    def audit_zonefit(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's ninth, opt-in pass, beside the gate (include/ksolve.h KS_AUDIT_POD_ZFIT_*, kshost.h ksh_audit_zonefit / ksh_audit_zonefit_claimed): first-fit order for
        the pods whose constraining groups are all eligible zonal spread groups, from the final state and the prefix counts at each pod's commit number.  Arguments as
        `audit_topology`'s.  Returns `audit_hostfit`'s dict ("checked": SEQ, PODS, ZONE the (pod, node) pairs whose zone test ran, STATIC those that passed it) plus
        "mixed_pods" and "exact_pods"."""
        return _audit("zonefit", [self], claimed, pod_seq)[0]

    def audit_stages(self, claimed: Optional[dict] = None, pod_seq=None) -> dict:
        """The audit's seventh, opt-in pass (include/ksolve.h KS_AUDIT_POD_STAGE_*, kshost.h ksh_audit_stages / ksh_audit_stages_claimed): relaxation order -- no pod ended
        at a later stage of its chain than one at which an existing node's final state or a fresh machine of an unlimited template admits it, and no unscheduled pod
        stopped short of its chain's end.  The gate runs it when `passes` names "stages".  Arguments as `audit_topology`'s.  Returns `audit_firstfit`'s dict ("checked": SEQ, PODS the
        pods with an examined earlier stage, STAGES those stages, PAIRS the (class, node-or-template) pairs)."""
        return _audit("stages", [self], claimed, pod_seq)[0]

    def audit_reasons(self, claimed: Optional[dict] = None) -> dict:
        """The audit's eighth, opt-in pass (include/ksolve.h KS_AUDIT_POD_REASON_*, kshost.h ksh_audit_reasons / ksh_audit_reasons_claimed): the failure reasons -- a
        placed pod carries no word, an unscheduled pod a KS_WHY_* nibble for each of the first eight templates, and where the flat problem alone decides the nibble
        (taints, requirements, no instance type) it is that value.  The gate runs it when `passes` names "reasons".  `claimed`: a result in `result_arrays()`' form, of which
        pod_node, pod_stage and pod_reason are read; no commit numbers.  Returns {"pod_flags", "n_pods_flagged", "pod_bit_count", "checked": PODS the unscheduled
        pods examined, EXACT / BOUNDED / UNEXAMINED their nibbles, "skipped_pods", "n_unscheduled", "used_classes", "pairs", "n_new", "n_placed", "ms"}."""
        return _audit("reasons", [self], claimed)[0]

    def audit_gate(self, claimed: Optional[dict] = None, pod_seq=None, passes=None, cap_findings: int = 1024, findings_table=None) -> dict:
        """The audit's gate (include/ksolve.h KS_AUDIT_PASS_*, kshost.h ksh_audit_gate / ksh_audit_gate_claimed): the passes named in `passes` (default: all six; "stages" and "reasons" may be named too, scheduler.AUDIT_GATE_ALL) in one
        call, tallied on the device -- no flag row is read back.  Arguments as `audit_topology`'s.  Returns `scheduler.audit_gate`'s dict, "passes" holding one dict per
        pass: what the pass's own method returns, without its flag arrays."""
        g = audit_gate([self], passes, cap_findings, claimed, pod_seq, findings_table)
        g["passes"] = {w: v[0] for w, v in g["passes"].items()}
        return g

    def result(self) -> SolveResult:
        """Decode the result the handle holds (after `solve(decode=False)` or `solve_from_pods`)."""
        kh = libs()[1]
        out = ctypes.c_void_p()
        rc = kh.ksh_result_text(self._h, ctypes.byref(out))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        text = ctypes.string_at(out).decode()
        kh.ksh_free(out)
        return parse_result(text)

    def grid(self, want_bits: bool = True):
        """ks_feasibility_grid: returns (numpy uint64 [M, C, TW] or None, kernel milliseconds)."""
        import numpy as np
        kh = libs()[1]
        tw = (self.dims["T"] + 63) // 64
        arr = np.zeros((self.dims["M"], self.dims["C"], tw), dtype=np.uint64) if want_bits else None
        ms = ctypes.c_float()
        rc = kh.ksh_grid(self._h, arr.ctypes.data if arr is not None else None, ctypes.byref(ms))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return arr, float(ms.value)

    def built_grid(self):
        """ksh_debug_grid: the grid as the last build left it -- this handle's own, or the batch's it was solved in (`grid()` rebuilds before it copies) -- as numpy
        uint64 [M, C, TW].  Read-only, nothing is launched; raises KS_ERR_INVALID before an upload or while the grid is not built."""
        import numpy as np
        kh = libs()[1]
        arr = np.zeros((self.dims["M"], self.dims["C"], (self.dims["T"] + 63) // 64), dtype=np.uint64)
        rc = kh.ksh_debug_grid(self._h, arr.ctypes.data)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return arr

    def whatif_topology(self):
        """ksh_debug_whatif_topology: what the derivation left this derived what-if with, as numpy arrays (active uint8 [G], count int32 [G, 64], extra int32 [GH]).
        Read-only, nothing is launched; raises KS_ERR_INVALID for a handle that is no derived what-if over a snapshot with topology groups."""
        import numpy as np
        kh = libs()[1]
        G, GH = self.dims["G"], self.dims["GH"]
        active, count, extra = np.zeros(max(1, G), dtype=np.uint8), np.zeros((max(1, G), 64), dtype=np.int32), np.zeros(max(1, GH), dtype=np.int32)
        rc = kh.ksh_debug_whatif_topology(self._h, active.ctypes.data, count.ctypes.data, extra.ctypes.data)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return active[:G], count[:G], extra[:GH]

    def arena_bytes(self) -> int:
        """ksh_whatifs_arena_bytes: device bytes of the arena a derived what-if's batch shares; 0 for a handle flattened on the host."""
        return int(libs()[1].ksh_whatifs_arena_bytes(self._h))

    def upload_bytes(self) -> int:
        """ksh_whatifs_upload_bytes: the bytes the open of a derived what-if's batch copied to the device; 0 for a handle flattened on the host."""
        return int(libs()[1].ksh_whatifs_upload_bytes(self._h))

    def pod_classes(self):
        """ksh_debug_pod_classes: numpy uint32 [P], the pod class (grid row c) of every pod as submitted, in the caller's pod order."""
        import numpy as np
        kh = libs()[1]
        arr = np.zeros(max(1, self.dims["P"]), dtype=np.uint32)
        rc = kh.ksh_debug_pod_classes(self._h, arr.ctypes.data)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return arr[:self.dims["P"]]

    def class_tables(self):
        """ksh_debug_classes: (briefs, plans), ctypes arrays of `ClsBrief` / `ClsPlan` [C], row c = pod class c (`pod_classes()` maps pods to rows) -- the records the pack
        kernels take their shortcuts from, as the last build left them: this handle's own (`grid()` rebuilds), or the batch's it was solved in.  Uploads the problem
        if it is not resident and builds the tables only if nothing has built them yet.  The mirrors' sizes are checked against the library's: a layout that
        drifted is an error, never a misread."""
        kh = libs()[1]
        assert ctypes.sizeof(ClsBrief) == 128, ctypes.sizeof(ClsBrief)
        C = self.dims["C"]
        briefs, plans = (ClsBrief * max(1, C))(), (ClsPlan * max(1, C))()
        rc = kh.ksh_debug_classes(self._h, None, None)
        if rc == KS_ERR_INVALID:      # not resident yet
            self.upload()
            rc = kh.ksh_debug_classes(self._h, None, None)
        if rc < 0:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        assert rc == ctypes.sizeof(ClsPlan), f"ClsPlan is {rc} bytes in the library, {ctypes.sizeof(ClsPlan)} in the Python mirror"
        rc = kh.ksh_debug_classes(self._h, ctypes.byref(briefs), ctypes.byref(plans))
        if rc < 0:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return briefs, plans

    def grid_rows(self, lo: int, hi: int, dev_ptr: int = 0):
        """ksh_grid_rows: rows [lo, hi) of the M * C grid rows computed on this handle's device; returns (numpy uint64 [hi - lo, TW], kernel ms).  dev_ptr: also
        copied device to device to that address (a slice of an all-gather's buffer)."""
        import numpy as np
        kh = libs()[1]
        tw = (self.dims["T"] + 63) // 64
        arr = np.zeros((hi - lo, tw), dtype=np.uint64)
        ms = ctypes.c_float()
        rc = kh.ksh_grid_rows(self._h, ctypes.c_uint32(lo), ctypes.c_uint32(hi), ctypes.c_void_p(arr.ctypes.data if hi > lo else None), ctypes.c_void_p(dev_ptr or None), ctypes.byref(ms))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return arr, float(ms.value)

    def grid_install(self, lo: int, hi: int, rows=None, dev_ptr: int = 0, complete: bool = False):
        """ksh_grid_install: rows computed elsewhere put in place (numpy uint64 [hi - lo, TW] or a device address); complete: every row is in."""
        import numpy as np
        kh = libs()[1]
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.uint64)
        rc = kh.ksh_grid_install(self._h, ctypes.c_uint32(lo), ctypes.c_uint32(hi), ctypes.c_void_p(rows.ctypes.data if rows is not None and hi > lo else None), ctypes.c_void_p(dev_ptr or None),
                                 ctypes.c_int(1 if complete else 0))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())


def sharded_grid(fp: "FlatProblem", rank: int, world: int, all_gather):
    """the static feasibility grid of a Solve built by `world` GPUs -- rank r computes rows [r * MC / world, (r + 1) * MC / world) of the M * C grid rows on ITS
    device from its copy of the (small) class and catalogue tables, ONE all-gather of the bit-rows (`all_gather(numpy rows of this rank) -> list of every rank's rows, in rank
    order`: torch.distributed over RCCL / gloo in bench.py and the tests), every rank installs the others' rows.  Returns the kernel milliseconds of this rank's share."""
    mc = fp.dims["M"] * fp.dims["C"]
    cut = [mc * r // world for r in range(world + 1)]
    rows, ms = fp.grid_rows(cut[rank], cut[rank + 1])
    parts = all_gather(rows)
    for r, part in enumerate(parts):
        if r != rank:
            fp.grid_install(cut[r], cut[r + 1], rows=part)
    fp.grid_install(0, 0, complete=True)
    return ms


class ParsedProblem:
    """The problem as C++ objects in host memory (ksh_parse) -- the analogue of the []*v1.Pod, []*cloudprovider.InstanceType and
    []*state.Node a Go caller holds when it calls NewScheduler / Solve.  `solve_from_pods` starts from here."""

    def __init__(self, problem: Optional[Problem], _text: Optional[bytes] = None):
        kh = libs()[1]
        text = _text if _text is not None else problem.to_ksp().encode()
        self._p = ctypes.c_void_p()
        rc = kh.ksh_parse(text, len(text), ctypes.byref(self._p))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())

    @classmethod
    def from_text(cls, ksp_text: bytes) -> "ParsedProblem":
        return cls(None, _text=ksp_text)

    @classmethod
    def from_env_block(cls, block: dict) -> "ParsedProblem":
        """The environment through the binary door (`ksh_env_ingest`; block from `model.env_to_block`): no KSP1 text on the way.  `ingest_ms`: the library's time."""
        kh = libs()[1]
        eb = _EnvBlock(block["n_strings"], block["n_words"], block["str_off"].ctypes.data, block["str_bytes"].ctypes.data, block["words"].ctypes.data,
                       int(block.get("str_bytes_len", block["str_bytes"].size)))
        self = cls.__new__(cls)
        self._p = ctypes.c_void_p()
        ms = ctypes.c_double()
        rc = kh.ksh_env_ingest(ctypes.byref(eb), ctypes.byref(self._p), ctypes.byref(ms))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        self.ingest_ms = float(ms.value)
        return self

    def apply(self, events: Sequence[tuple], pod_node: Optional[Sequence[int]] = None) -> dict:
        """Keep the snapshot current by events instead of ingesting it again (kshost.h `ksh_env_apply`; state.Cluster's UpdateNode / DeleteNode / UpdatePod /
        DeletePod, cluster.go): `events` as `model.delta_to_ksd` takes them.  The first call needs the snapshot's bindings (`pod_node`); from then on the library
        holds them (`bindings()`), and `open_whatifs(..., pod_node=None)` means those.  Returns {"applied", "nodes", "pods", "continued", "ms"}: `continued` says the
        snapshot's flattening took the short road (same universes), `ms` is the library's time for events + flattening.  ("IT=", InstanceType) replaces the
        instance type of that name in place -- offerings, prices, requirements, capacity, overhead -- and keeps its index."""
        import numpy as np, time
        from .model import delta_to_ksd
        kh = libs()[1]
        text = delta_to_ksd(events).encode()
        pn = None if pod_node is None else np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32))
        info = (ctypes.c_uint32 * 4)()
        kh.ksh_env_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32)]
        t0 = time.perf_counter()
        rc = kh.ksh_env_apply(self._p, None if pn is None or pn.size == 0 else pn.ctypes.data, text, len(text), info)
        ms = (time.perf_counter() - t0) * 1e3
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return {"applied": int(info[0]), "nodes": int(info[1]), "pods": int(info[2]), "continued": bool(info[3]), "ms": ms}

    def apply_block(self, events, pod_node: Optional[Sequence[int]] = None, track_cluster_pods: bool = False) -> dict:
        """`apply` through the binary door (kshost.h `ksh_env_apply_block`): the same events (or the block `model.delta_to_block` made of them, for a caller that
        builds it ahead of the call), no KSD1 text on the way, the same returned dict.  A malformed block applies nothing.  `track_cluster_pods`
        (KSH_APPLY_TRACK_CLUSTER_PODS): mirror BIND / UNBIND into the snapshot's cluster pods even if it had none at the first call -- what a topology-tracking
        snapshot that starts with no bound pod needs.  A refused call raises KSolveError carrying `.info`: the same dict, saying what was applied before the refusal."""
        import numpy as np, time
        from .model import delta_to_block
        kh = libs()[1]
        b = events if isinstance(events, dict) else delta_to_block(events)
        db = _DeltaBlock(b["n_events"], b["n_strings"], b["n_words"], b["str_off"].ctypes.data, b["str_bytes"].ctypes.data, b["words"].ctypes.data,
                         int(b.get("str_bytes_len", b["str_bytes"].size)))
        pn = None if pod_node is None else np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32))
        info = (ctypes.c_uint32 * 4)()
        kh.ksh_env_apply_block.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        t0 = time.perf_counter()
        rc = kh.ksh_env_apply_block(self._p, None if pn is None or pn.size == 0 else pn.ctypes.data, ctypes.byref(db), KSH_APPLY_TRACK_CLUSTER_PODS if track_cluster_pods else 0, info)
        ms = (time.perf_counter() - t0) * 1e3
        out = {"applied": int(info[0]), "nodes": int(info[1]), "pods": int(info[2]), "continued": bool(info[3]), "ms": ms}
        if rc != KS_OK:
            err = KSolveError(rc, kh.ksh_last_error().decode())
            err.info = out
            raise err
        return out

    def bindings(self):
        """(pod -> node index, -1 for a pod that was unbound; number of node slots) as the library holds them after `apply`."""
        import numpy as np
        kh = libs()[1]
        kh.ksh_snapshot_bindings.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
        n_pods, n_nodes = ctypes.c_uint32(), ctypes.c_uint32()
        if kh.ksh_snapshot_bindings(self._p, None, 0, ctypes.byref(n_pods), ctypes.byref(n_nodes)) != KS_OK:
            raise KSolveError(KS_ERR_INVALID, kh.ksh_last_error().decode())
        out = np.full(max(1, n_pods.value), -1, dtype=np.int32)
        rc = kh.ksh_snapshot_bindings(self._p, out.ctypes.data, n_pods.value, None, None)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return out[:n_pods.value], int(n_nodes.value)

    def snapshot_fingerprint(self, pod_node: Optional[Sequence[int]] = None, cold: bool = False, volumes: bool = False, active_resources: bool = False,
                             group_lists: bool = False) -> int:
        """Hash of the snapshot's flattening (flat problem + the tables the device derivation reads); `cold`: of one made from scratch (tests: a flattening
        continued after `apply` must equal it); `volumes`: of the flattening derived what-ifs with volumes use (KSH_DERIVE_VOLUMES);
        `active_resources`: of the flattening over the active resource names (KSH_ACTIVE_RESOURCES)."""
        import numpy as np
        kh = libs()[1]
        kh.ksh_snapshot_fingerprint.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        pn = None if pod_node is None else np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32))
        out = ctypes.c_uint64()
        rc = kh.ksh_snapshot_fingerprint(self._p, None if pn is None or pn.size == 0 else pn.ctypes.data, (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | (KSH_DERIVE_GROUP_LISTS if group_lists else 0), 1 if cold else 0, ctypes.byref(out))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return int(out.value)

    def close(self):
        if self._p:
            libs()[1].ksh_parsed_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TIMING_KEYS = ("flatten_ms", "upload_ms", "tables_grid_ms", "pack_kernel_ms", "solve_readback_ms", "total_ms")


def solve_from_pods(parsed: ParsedProblem, device: int = 0, stats: bool = False, keep: bool = True, active_resources: bool = False):
    """Everything the reference does inside NewScheduler + Solve for a pod list it already holds: flatten (incl. NewQueue's
    sort, per-pod requests / requirements / classes / relaxation chains), upload, static tables + feasibility grid, the pack
    kernel, read-back.  Returns (FlatProblem holding the result or None, timings dict in milliseconds)."""
    kh = libs()[1]
    h = ctypes.c_void_p()
    ms = (ctypes.c_double * 6)()
    rc = kh.ksh_solve_from_pods(parsed._p, device, (KS_FLAG_STATS if stats else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0), ctypes.byref(h) if keep else None, ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    fp = FlatProblem(None, _handle=h) if keep else None
    if fp is not None:
        fp.kernel_ms = float(ms[3])
    return fp, dict(zip(TIMING_KEYS, [float(x) for x in ms]))


class _PodBlock(ctypes.Structure):      # include/kshost.h ksh_pod_block
    _fields_ = [("n_pods", ctypes.c_uint32), ("n_strings", ctypes.c_uint32), ("str_off", ctypes.c_void_p), ("str_bytes", ctypes.c_void_p),
                ("spec_off", ctypes.c_void_p), ("spec_words", ctypes.c_void_p), ("uid", ctypes.c_void_p), ("creation_ts", ctypes.c_void_p),
                ("str_bytes_len", ctypes.c_uint64), ("spec_words_len", ctypes.c_uint64)]


class _EnvBlock(ctypes.Structure):
    _fields_ = [("n_strings", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("str_off", ctypes.c_void_p), ("str_bytes", ctypes.c_void_p), ("words", ctypes.c_void_p), ("str_bytes_len", ctypes.c_uint64)]


class _DeltaBlock(ctypes.Structure):      # include/kshost.h ksh_delta_block
    _fields_ = [("n_events", ctypes.c_uint32), ("n_strings", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("str_off", ctypes.c_void_p), ("str_bytes", ctypes.c_void_p),
                ("words", ctypes.c_void_p), ("str_bytes_len", ctypes.c_uint64)]


class PodBatch:
    """The pending pods handed over as flat arrays (`ksh_pods_ingest`; blocks from `model.pods_to_blocks`) -- the binary door a cgo shim would
    use instead of KSP1 text.  `ingest_ms` is the library's time to take the blocks in (hash, partition, decode the distinct specs)."""

    def __init__(self, blocks: Sequence[dict]):
        kh = libs()[1]
        arr = (_PodBlock * max(1, len(blocks)))()
        for i, b in enumerate(blocks):
            arr[i] = _PodBlock(b["n_pods"], b["n_strings"], b["str_off"].ctypes.data, b["str_bytes"].ctypes.data, b["spec_off"].ctypes.data,
                               b["spec_words"].ctypes.data, b["uid"].ctypes.data, b["creation_ts"].ctypes.data,
                               int(b.get("str_bytes_len", b["str_bytes"].size)), int(b.get("spec_words_len", b["spec_words"].size)))
        self._b = ctypes.c_void_p()
        ms = ctypes.c_double()
        rc = kh.ksh_pods_ingest(ctypes.cast(arr, ctypes.c_void_p), len(blocks), ctypes.byref(self._b), ctypes.byref(ms))
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        self.ingest_ms = float(ms.value)
        n, s = ctypes.c_uint32(), ctypes.c_uint32()
        kh.ksh_pods_count(self._b, ctypes.byref(n), ctypes.byref(s))
        self.n_pods, self.n_specs = int(n.value), int(s.value)

    def close(self):
        if self._b:
            libs()[1].ksh_pods_free(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def open_batch(env: ParsedProblem, batch: PodBatch, stats: bool = False, active_resources: bool = False) -> FlatProblem:
    """Flatten `batch` against the environment `env` (a ParsedProblem of a Problem WITHOUT pods): host side only, like FlatProblem(problem)."""
    kh = libs()[1]
    h = ctypes.c_void_p()
    rc = kh.ksh_open_batch(env._p, batch._b, (KS_FLAG_STATS if stats else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0), ctypes.byref(h))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return FlatProblem(None, _handle=h)


def solve_from_batch(env: ParsedProblem, batch: PodBatch, device: int = 0, stats: bool = False, keep: bool = True, active_resources: bool = False):
    """`solve_from_pods` for a batch that came in through the binary door."""
    kh = libs()[1]
    h = ctypes.c_void_p()
    ms = (ctypes.c_double * 6)()
    rc = kh.ksh_solve_from_batch(env._p, batch._b, device, (KS_FLAG_STATS if stats else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0), ctypes.byref(h) if keep else None, ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    fp = FlatProblem(None, _handle=h) if keep else None
    if fp is not None:
        fp.kernel_ms = float(ms[3])
    return fp, dict(zip(TIMING_KEYS, [float(x) for x in ms]))


def open_whatifs(snapshot, pod_node: Sequence[int], candidate_sets: Sequence[Sequence[int]], threads: int = 0, stats: bool = False, derive=None, device: int = 0,
                 volumes: bool = False, active_resources: bool = False, group_lists: bool = False) -> List[FlatProblem]:
    """Flatten N consolidation what-ifs over one cluster snapshot natively (simulateScheduling, deprovisioning/helpers.go:42-115):
    `snapshot` (a `Problem`, or a `ParsedProblem` already held as objects) lists every state node and, as its pod batch, every bound pod
    (full spec); pod_node[i] = node index of pod i.  What-if w removes candidate_sets[w] from the state nodes and makes their pods
    (candidate order, then pod order) the pending batch.  The snapshot is flattened ONCE; the per-what-if part (its pods' classes, queue and
    topology groups, remainingResources) runs on `threads` host threads (0 = all usable cores)."""
    kh = libs()[1]
    n = len(candidate_sets)
    import numpy as np
    lens = np.fromiter((len(cs) for cs in candidate_sets), dtype=np.int64, count=n)
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum(lens, out=off[1:])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(cs, dtype=np.uint32) for cs in candidate_sets]) if n else np.zeros(1, dtype=np.uint32))
    if flat.size == 0:
        flat = np.zeros(1, dtype=np.uint32)
    # pod_node None: the bindings the library holds itself since `ParsedProblem.apply`
    pn = None if pod_node is None else (np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32)) if len(pod_node) else np.zeros(1, dtype=np.int32))
    c_off = off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    c_cand = flat.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    c_pn = None if pn is None else pn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    hs = (ctypes.c_void_p * max(1, n))()
    act = KSH_ACTIVE_RESOURCES if active_resources else 0      # (kshost.h: the snapshot flattened over the names its bound pods, daemonsets and limits name)
    # derive: None = derive the what-ifs on the device when the snapshot allows it (a ParsedProblem without topology terms / volume limits), else flatten
    # them one by one on the host; True = derive or raise; False = always flatten on the host.  Derived what-ifs are resident on `device` at once.
    # volumes: opt in to deriving snapshots with CSI volume limits / claims too (kshost.h KSH_DERIVE_VOLUMES); the host route is the same either way.
    # group_lists: opt in to the per-node lists behind a derived what-if's topology (kshost.h KSH_DERIVE_GROUP_LISTS): more than 1024 topology groups are derived too.
    if derive is not False and not stats and n:
        if not isinstance(snapshot, ParsedProblem):
            snapshot = ParsedProblem(snapshot)       # (the handles keep what they need of it alive)
        rc = kh.ksh_open_whatifs_derived(snapshot._p, (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_DERIVE_GROUP_LISTS if group_lists else 0) | act, n, c_off, c_cand, c_pn, device, hs)
        if rc == KS_OK:
            return [FlatProblem(None, _handle=ctypes.c_void_p(hs[i])) for i in range(n)]
        if derive is True or rc not in (KS_ERR_UNSUPPORTED, KS_ERR_DEVICE):
            raise KSolveError(rc, kh.ksh_last_error().decode())
    elif derive is True:
        raise KSolveError(KS_ERR_UNSUPPORTED, "derived what-ifs carry no reference-algorithm statistics")
    if isinstance(snapshot, ParsedProblem):
        rc = kh.ksh_open_whatifs_parsed(snapshot._p, (KS_FLAG_STATS if stats else 0) | act, n, c_off, c_cand, c_pn, threads, hs)
    else:
        text = snapshot.to_ksp().encode()
        rc = kh.ksh_open_whatifs(text, len(text), (KS_FLAG_STATS if stats else 0) | act, n, c_off, c_cand, c_pn, threads, hs)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return [FlatProblem(None, _handle=ctypes.c_void_p(hs[i])) for i in range(n)]


def check_whatif_derivation(snapshot: "ParsedProblem", pod_node: Sequence[int], candidates: Sequence[int], volumes: bool = False, active_resources: bool = False,
                            group_lists: bool = False) -> None:
    """Diagnostic, no GPU needed (kshost.h `ksh_check_whatif_derivation`): what the device would derive for this candidate set -- group activity, domain
    counts, hostname rows; with `volumes`, the volume state of every node that stays and the volume test of every pod of the batch on it -- restated on
    the host and compared with the what-if flattened by itself.  Raises KSolveError with the first difference."""
    import numpy as np
    kh = libs()[1]
    cand = np.ascontiguousarray(np.asarray(list(candidates) or [0], dtype=np.uint32))
    pn = None if pod_node is None else (np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32)) if len(pod_node) else np.zeros(1, dtype=np.int32))
    kh.ksh_check_whatif_derivation.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)]
    rc = kh.ksh_check_whatif_derivation(snapshot._p, (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | (KSH_DERIVE_GROUP_LISTS if group_lists else 0), cand.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(candidates), None if pn is None else pn.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())


def solve_batch(flats: Sequence[FlatProblem], decode: bool = True):
    """N independent Solve() calls in one launch (consolidation what-ifs)."""
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    outs = (ctypes.c_void_p * n)()
    kms, wms = ctypes.c_float(), ctypes.c_double()
    rc = kh.ksh_solve_batch(hs, n, outs if decode else None, ctypes.byref(kms), ctypes.byref(wms))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    res = None
    if decode:
        res = []
        for i in range(n):
            res.append(parse_result(ctypes.string_at(outs[i]).decode()))
            kh.ksh_free(outs[i])
    return res, float(kms.value), float(wms.value)


class _ResultArrays(ctypes.Structure):      # include/kshost.h ksh_result_arrays
    _fields_ = [(n, ctypes.c_uint32) for n in ("n_pods", "n_existing", "n_new", "n_unscheduled", "types_words", "n_resources", "n_keys", "pad")] + \
               [(n, ctypes.c_void_p) for n in ("pod_node", "pod_stage", "pod_reason", "unscheduled", "node_pods_off", "node_pods", "node_tmpl", "node_types", "node_requests",
                                               "node_requests_present", "node_present", "node_complement", "node_mask", "node_gt", "node_lt", "node_it_state")]


# The claimed arrays every pass uploads, and the two sets some read beyond them (name, dtype: the fields of _ResultArrays).
_CLAIMED_COMMON = (("pod_node", "int32"), ("pod_stage", "int32"), ("node_tmpl", "int32"), ("node_present", "uint32"), ("node_complement", "uint32"), ("node_mask", "uint64"),
                   ("node_gt", "int32"), ("node_lt", "int32"))
_CLAIMED_FIT = (("node_types", "uint64"), ("node_requests", "int64"), ("node_requests_present", "uint32"), ("node_it_state", "int32"))
_CLAIMED_FIRST = (("unscheduled", "int32"),) + _CLAIMED_FIT

# The audit's passes: what differs between them and nothing else.  stem: the C name (kshost.h <stem> / <stem>_claimed);  seq: the claimed form takes the commit numbers;
# fields: the uint32 members of <stem>_out behind its tables ("name*N": an array of N) -- a bit count the struct holds is read from it, one it lacks is counted from the flags;
# claimed: what a claimed result uploads beyond _CLAIMED_COMMON;  node_bits: the pass has a table per node as well;  checked: the names of `checked`' entries;
# scalars: the members returned as they are, in the dict's order.
_AUDIT_PASSES = {
    "audit": dict(stem="ksh_audit", seq=False, out="_AuditOut", claimed=_CLAIMED_FIRST, pod_bits=KS_AUDIT_POD_BITS, node_bits=KS_AUDIT_NODE_BITS, checked=None,
                  fields=("n_pods", "n_nodes", "n_new", "n_unscheduled", "n_pods_flagged", "n_nodes_flagged", "truncated", "pad", "pod_bit_count*32", "node_bit_count*32"),
                  scalars=("n_new", "n_unscheduled")),
    "topology": dict(stem="ksh_audit_topology", seq=True, out="_AuditTopologyOut", claimed=(), pod_bits=KS_AUDIT_TOPOLOGY_BITS, node_bits=None, checked=KS_AUDIT_TOPOLOGY_RULES,
                     fields=("n_pods", "n_new", "n_placed", "skipped_groups", "n_pods_flagged", "truncated", "checked*4", "pod_bit_count*32"),
                     scalars=("skipped_groups", "n_new", "n_placed")),
    "spread": dict(stem="ksh_audit_spread", seq=True, out="_AuditSpreadOut", claimed=(), pod_bits=KS_AUDIT_SPREAD_BITS, node_bits=None, checked=KS_AUDIT_SPREAD_RULES,
                   fields=("n_pods", "n_new", "n_placed", "skipped_groups", "n_pods_flagged", "truncated", "checked*2", "exact_pairs", "pad"),
                   scalars=("exact_pairs", "skipped_groups", "n_new", "n_placed")),
    "firstfit": dict(stem="ksh_audit_firstfit", seq=True, out="_AuditFirstFitOut", claimed=_CLAIMED_FIT, pod_bits=KS_AUDIT_FIRSTFIT_BITS, node_bits=None, checked=KS_AUDIT_FIRSTFIT_CHECKED,
                     fields=("n_pods", "n_new", "n_placed", "skipped_pods", "n_pods_flagged", "truncated", "checked*3", "admitting_pairs"),
                     scalars=("admitting_pairs", "skipped_pods", "n_new", "n_placed")),
    "limits": dict(stem="ksh_audit_limits", seq=True, out="_AuditLimitsOut", claimed=_CLAIMED_FIT, pod_bits=KS_AUDIT_LIMITS_POD_BITS, node_bits=KS_AUDIT_LIMITS_NODE_BITS,
                   checked=KS_AUDIT_LIMITS_CHECKED,
                   fields=("n_pods", "n_nodes", "n_new", "n_placed", "limited_templates", "skipped_nodes", "skipped_pods", "truncated", "n_pods_flagged", "n_nodes_flagged",
                           "exact_nodes", "binding_nodes", "checked*4", "pod_bit_count*32", "node_bit_count*32"),
                   scalars=("limited_templates", "exact_nodes", "binding_nodes", "skipped_nodes", "skipped_pods", "n_new", "n_placed")),
    "hostfit": dict(stem="ksh_audit_hostfit", seq=True, out="_AuditHostFitOut", claimed=_CLAIMED_FIT, pod_bits=KS_AUDIT_HOSTFIT_BITS, node_bits=None, checked=KS_AUDIT_HOSTFIT_CHECKED,
                    fields=("n_pods", "n_new", "n_placed", "skipped_pods", "n_pods_flagged", "truncated", "eligible_groups", "skipped_groups", "checked*4", "admitting_pairs", "pad"),
                    scalars=("admitting_pairs", "skipped_pods", "eligible_groups", "skipped_groups", "n_new", "n_placed")),
}

# The pass beside the six (the gate runs it through its wide form, _AUDIT_PASSES_EX below): described as the ones above and called through the same _audit(), but outside _AUDIT_PASSES, whose places are the gate's mask
# bits and the members of its struct.
_AUDIT_PASSES_BESIDE = {
    "stages": dict(stem="ksh_audit_stages", seq=True, out="_AuditStagesOut", claimed=_CLAIMED_FIT, pod_bits=KS_AUDIT_STAGES_BITS, node_bits=None, checked=KS_AUDIT_STAGES_CHECKED,
                   fields=("n_pods", "n_new", "n_placed", "skipped_pods", "n_pods_flagged", "truncated", "checked*4", "admitting_pairs", "pad"),
                   scalars=("admitting_pairs", "skipped_pods", "n_new", "n_placed")),
}

# The pass over pod_reason: in the same form, in a table of its own -- the two above stay what they were.  Its claimed form reads pod_reason, which no other pass
# uploads, and takes no commit numbers.
_AUDIT_PASSES_REASONS = {
    "reasons": dict(stem="ksh_audit_reasons", seq=False, out="_AuditReasonsOut", claimed=(("pod_reason", "uint32"),), pod_bits=KS_AUDIT_REASONS_BITS, node_bits=None,
                    checked=KS_AUDIT_REASONS_CHECKED,
                    fields=("n_pods", "n_new", "n_placed", "n_unscheduled", "skipped_pods", "n_pods_flagged", "truncated", "used_classes", "checked*4", "pairs", "pad"),
                    scalars=("skipped_pods", "n_unscheduled", "used_classes", "pairs", "n_new", "n_placed")),
}

# The pass over zonal spread pods: in the same form, in a table of its own, beside the gate -- the three above, and everything derived from them, stay what they were.
_AUDIT_PASSES_ZONEFIT = {
    "zonefit": dict(stem="ksh_audit_zonefit", seq=True, out="_AuditZoneFitOut", claimed=_CLAIMED_FIT, pod_bits=KS_AUDIT_ZONEFIT_BITS, node_bits=None, checked=KS_AUDIT_ZONEFIT_CHECKED,
                    fields=("n_pods", "n_new", "n_placed", "skipped_pods", "n_pods_flagged", "truncated", "eligible_groups", "skipped_groups", "mixed_pods", "exact_pods", "checked*4",
                            "admitting_pairs", "pad"),
                    scalars=("admitting_pairs", "exact_pods", "skipped_pods", "mixed_pods", "eligible_groups", "skipped_groups", "n_new", "n_placed")),
}

for _p in list(_AUDIT_PASSES.values()) + list(_AUDIT_PASSES_BESIDE.values()) + list(_AUDIT_PASSES_REASONS.values()) + list(_AUDIT_PASSES_ZONEFIT.values()):      # include/kshost.h <stem>_out: the tables and their capacities, then `fields`
    _tables = [("pod_flags", ctypes.c_void_p), ("cap_pods", ctypes.c_uint64)] + ([("node_flags", ctypes.c_void_p), ("cap_nodes", ctypes.c_uint64)] if _p["node_bits"] else [])
    _p["Out"] = type(_p["out"], (ctypes.Structure,), {"_fields_": _tables + [(n, ctypes.c_uint32 * int(k) if k else ctypes.c_uint32) for n, _, k in (f.partition("*") for f in _p["fields"])]})
_AuditOut, _AuditTopologyOut, _AuditSpreadOut, _AuditFirstFitOut, _AuditLimitsOut, _AuditHostFitOut = (_AUDIT_PASSES[w]["Out"] for w in ("audit", "topology", "spread", "firstfit", "limits", "hostfit"))
_AuditStagesOut = _AUDIT_PASSES_BESIDE["stages"]["Out"]
_AuditReasonsOut = _AUDIT_PASSES_REASONS["reasons"]["Out"]
_AuditZoneFitOut = _AUDIT_PASSES_ZONEFIT["zonefit"]["Out"]


def _claimed_arrays(flat: "FlatProblem", claimed: dict, pod_seq, beyond, what: str):
    """ksh_result_arrays over the arrays of `claimed` that a pass uploads (_CLAIMED_COMMON and `beyond`), the commit numbers as an array of their own (or None), and what
    must stay alive for the call."""
    import numpy as np
    d, keep, seq = flat.dims, [], None
    ra = _ResultArrays()
    ra.n_pods, ra.n_existing, ra.n_new, ra.n_unscheduled = d["P"], d["E"], int(claimed["n_new"]), len(claimed["unscheduled"])
    ra.types_words, ra.n_resources, ra.n_keys = (d["T"] + 63) // 64, d["R"], d["K"]
    for name, dt in dict(_CLAIMED_COMMON + tuple(beyond)).items():
        a = np.ascontiguousarray(np.asarray(claimed[name], dtype=dt).reshape(-1))
        if not len(a):
            a = np.zeros(1, dtype=dt)      # (a table of no elements is still a table: never NULL)
        keep.append(a)
        setattr(ra, name, a.ctypes.data)
    if pod_seq is not None:
        seq = np.ascontiguousarray(np.asarray(pod_seq, dtype=np.int32).reshape(-1))
        if len(seq) != d["P"]:
            raise ValueError("audit_%s: pod_seq holds one commit number per pod" % what)
        if not len(seq):
            seq = np.zeros(1, dtype=np.int32)
    return ra, seq, keep


def _audit(what: str, flats: Sequence["FlatProblem"], claimed: Optional[dict] = None, pod_seq=None) -> List[dict]:
    """One pass of the audit, as _AUDIT_PASSES[what] (or _AUDIT_PASSES_BESIDE[what], _AUDIT_PASSES_REASONS[what] or, last, _AUDIT_PASSES_ZONEFIT[what]) states it: the call over the resident results of `flats`, or over `claimed` (with `pod_seq`, where the pass takes
    it) for flats[0]; once more with larger tables if one was too short.  One dict per problem."""
    import numpy as np
    if claimed is None and pod_seq is not None:
        raise ValueError("audit_%s: pod_seq goes with a claimed result" % what)
    n = len(flats)
    if not n:
        return []
    p, kh = _AUDIT_PASSES.get(what) or _AUDIT_PASSES_BESIDE.get(what) or _AUDIT_PASSES_REASONS.get(what) or _AUDIT_PASSES_ZONEFIT[what], libs()[1]
    Out, nodes = p["Out"], p["node_bits"] is not None
    resident, claimed_fn = getattr(kh, p["stem"]), getattr(kh, p["stem"] + "_claimed")
    resident.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_double)]
    claimed_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ResultArrays)] + [ctypes.c_void_p] * p["seq"] + [ctypes.POINTER(Out), ctypes.POINTER(ctypes.c_double)]
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    outs = (Out * n)()
    ms = (ctypes.c_double * 2)()
    ra = seq = None
    if claimed is not None:
        ra, seq, _keep = _claimed_arrays(flats[0], claimed, pod_seq, p["claimed"], what)

    def call(caps):
        tabs = []
        for o, (cp, cn) in zip(outs, caps):
            pf, nf = np.zeros(max(1, cp), dtype=np.uint32), np.zeros(max(1, cn), dtype=np.uint32) if nodes else None
            tabs.append((pf, nf))
            o.pod_flags, o.cap_pods = pf.ctypes.data, cp
            if nodes:
                o.node_flags, o.cap_nodes = nf.ctypes.data, cn
        if ra is None:
            rc = resident(hs, n, outs, ms)
        else:
            rc = claimed_fn(flats[0]._h, ctypes.byref(ra), *([seq.ctypes.data if seq is not None else None] * p["seq"]), outs, ms)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return tabs
    tabs = call([(f.dims["P"], f.dims["E"] + f.dims["P"]) for f in flats])
    if any(o.truncated for o in outs):      # (a table was too short -- a what-if derived on the device states its own sizes only here: once more, with what the totals say)
        tabs = call([(o.n_pods, o.n_nodes if nodes else 0) for o in outs])

    res = []
    for o, (pf, nf) in zip(outs, tabs):
        r = _audit_totals(p, o, pf[:o.n_pods].copy(), nf[:o.n_nodes].copy() if nodes else None)
        r["ms"] = (float(ms[0]), float(ms[1]))
        res.append(r)
    return res


def _audit_totals(p: dict, o, pf=None, nf=None) -> dict:
    """One problem's dict of the pass `p` of _AUDIT_PASSES from its out struct `o`.  pf / nf: its flag rows -- None from the gate, which reads none back: the dict
    then holds no flag array, and a bit count only where the struct carries it (the others are counted from the rows)."""
    nodes = p["node_bits"] is not None

    def bit_count(flags, field, bits):
        if hasattr(o, field):
            return {k: int(getattr(o, field)[v.bit_length() - 1]) for k, v in bits.items()}
        return None if flags is None else {k: int(((flags & v) != 0).sum()) for k, v in bits.items()}
    r = {}
    if pf is not None:
        r["pod_flags"] = pf
        if nodes:
            r["node_flags"] = nf
    r["n_pods_flagged"] = int(o.n_pods_flagged)
    if nodes:
        r["n_nodes_flagged"] = int(o.n_nodes_flagged)
    r["pod_bit_count"] = bit_count(pf, "pod_bit_count", p["pod_bits"])
    if nodes:
        r["node_bit_count"] = bit_count(nf, "node_bit_count", p["node_bits"])
    if r["pod_bit_count"] is None:
        del r["pod_bit_count"]
    if p["checked"]:
        r["checked"] = {k: int(o.checked[j]) for j, k in enumerate(p["checked"])}
    r.update((k, int(getattr(o, k))) for k in p["scalars"])
    return r


# The gate (include/kshost.h ksh_audit_gate / ksh_audit_gate_claimed, include/ksolve.h KS_AUDIT_PASS_*): a pass's mask bit is its place in _AUDIT_PASSES
KS_AUDIT_PASS = {name: 1 << i for i, name in enumerate(_AUDIT_PASSES)}
KS_AUDIT_GATE_TRUNCATED = 1
AUDIT_FINDING = [("problem", "<u4"), ("where", "<u4"), ("index", "<u4"), ("flags", "<u4")]      # ks_audit_finding; where = pass << 8 | table (0 pods, 1 nodes)


def audit_reduce_rows(rows, fields: Sequence[tuple] = (), device: int = 0) -> dict:
    """The gate's reduction over any table of words (include/ksolve.h ks_audit_reduce_rows): `rows` tallied on the device as a flag table -- {"n_set", "bit_count":
    [32]} -- and as a table of checked words with up to four `fields` (shift, mask): "field_sum": [sum of (row >> shift) & mask].  All sums modulo 2**32."""
    import numpy as np
    ks = libs()[0]
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.uint32).reshape(-1))
    f, out = (ctypes.c_uint32 * 9)(len(fields), *[int(s) for s, _ in fields], *([0] * (4 - len(fields))), *[int(m) for _, m in fields]), (ctypes.c_uint32 * 37)()
    ks.ks_audit_reduce_rows.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    rc = ks.ks_audit_reduce_rows(device, rows.ctypes.data if len(rows) else None, len(rows), f, out)
    if rc != KS_OK:
        ks.ks_last_error.restype = ctypes.c_char_p
        raise KSolveError(rc, ks.ks_last_error().decode())
    return {"n_set": int(out[0]), "bit_count": [int(x) for x in out[1:33]], "field_sum": [int(x) for x in out[33:33 + len(fields)]]}


class _AuditGateOut(ctypes.Structure):      # include/kshost.h ksh_audit_gate_out
    _fields_ = [("findings", ctypes.c_void_p), ("cap_findings", ctypes.c_uint64)] + [(name, ctypes.POINTER(p["Out"])) for name, p in _AUDIT_PASSES.items()] + \
               [("n_findings", ctypes.c_uint32), ("truncated", ctypes.c_uint32)]


# The gate over all eight passes (include/kshost.h ksh_audit_gate_ex / ksh_audit_gate_ex_claimed, include/ksolve.h KS_AUDIT_PASS_ALL_EX): the six tables above stay what
# they are; the wide form names the passes beside them too.  A pass's mask bit is its place in AUDIT_GATE_ALL.
_AUDIT_PASSES_EX = dict(_AUDIT_PASSES, **_AUDIT_PASSES_BESIDE, **_AUDIT_PASSES_REASONS)
AUDIT_GATE_ALL = tuple(_AUDIT_PASSES_EX)      # the eight names in mask order
KS_AUDIT_PASS_EX = {name: 1 << i for i, name in enumerate(AUDIT_GATE_ALL)}


class _AuditGateExOut(ctypes.Structure):      # include/kshost.h ksh_audit_gate_ex_out: struct_size leads, the passes after the sixth have their pointers at the end
    _fields_ = [("struct_size", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("findings", ctypes.c_void_p), ("cap_findings", ctypes.c_uint64)] + \
               [(name, ctypes.POINTER(p["Out"])) for name, p in _AUDIT_PASSES.items()] + [("n_findings", ctypes.c_uint32), ("truncated", ctypes.c_uint32)] + \
               [(name, ctypes.POINTER(_AUDIT_PASSES_EX[name]["Out"])) for name in AUDIT_GATE_ALL[len(_AUDIT_PASSES):]]


def audit_gate(flats: Sequence["FlatProblem"], passes: Optional[Sequence[str]] = None, cap_findings: int = 1024, claimed: Optional[dict] = None, pod_seq=None,
               findings_table=None, wide: Optional[bool] = None) -> dict:
    """The audit's gate (include/kshost.h ksh_audit_gate): the passes named in `passes` (default: all six of _AUDIT_PASSES) over the resident results of `flats` in one
    call -- or over `claimed` with `pod_seq` for flats[0] --, tallied on the device: no flag row is read back.  Returns {"clean": no pass found anything, "passes":
    {name: one dict per problem, as the pass's own call returns it without its flag arrays}, "findings": a structured array (AUDIT_FINDING) of the first
    min(n_findings, cap_findings) non-zero flag words, ordered by pass, problem, pods before nodes, index, "n_findings": all of them, "truncated", "ms"}.
    findings_table: an array of `cap_findings` AUDIT_FINDING records to write into (a caller who wants to see what is left untouched).
    `passes` may name "stages" and "reasons" too (AUDIT_GATE_ALL: all eight): the call then goes through the wide gate (ksh_audit_gate_ex), "passes" comes back in
    mask order, a claimed result carries `pod_reason` when "reasons" is named, and `pod_seq` may be left out when only "audit" and "reasons" are.  wide=True sends
    a mask of the six through the wide gate as well (it answers what the old one answers); wide=None decides by the names."""
    import numpy as np
    names = list(_AUDIT_PASSES) if passes is None else list(passes)
    if wide is None:
        wide = any(w not in _AUDIT_PASSES and w in KS_AUDIT_PASS_EX for w in names)
    if wide:
        names = [w for w in AUDIT_GATE_ALL if w in names] + [w for w in names if w not in KS_AUDIT_PASS_EX]      # (an unknown name: the KeyError below)
    table_of, bit_of = (_AUDIT_PASSES_EX, KS_AUDIT_PASS_EX) if wide else (_AUDIT_PASSES, KS_AUDIT_PASS)
    mask = 0
    for w in names:
        mask |= bit_of[w]
    n, kh = len(flats), libs()[1]
    Gate, stem = (_AuditGateExOut, "ksh_audit_gate_ex") if wide else (_AuditGateOut, "ksh_audit_gate")
    out = Gate()
    if wide:
        out.struct_size = ctypes.sizeof(Gate)
    table = np.zeros(max(1, cap_findings), dtype=AUDIT_FINDING) if findings_table is None else findings_table
    out.findings, out.cap_findings = (table.ctypes.data if cap_findings else None), cap_findings
    outs = {w: (table_of[w]["Out"] * max(1, n))() for w in names}
    for w, a in outs.items():
        setattr(out, w, a)
    ms = (ctypes.c_double * 2)()
    if claimed is None:
        if pod_seq is not None:
            raise ValueError("audit_gate: pod_seq goes with a claimed result")
        resident = getattr(kh, stem)
        resident.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Gate), ctypes.POINTER(ctypes.c_double)]
        rc = resident((ctypes.c_void_p * max(1, n))(*[f._h for f in flats]), n, mask, ctypes.byref(out), ms)
    else:
        ra, seq, _keep = _claimed_arrays(flats[0], claimed, pod_seq, sum((table_of[w]["claimed"] for w in names), ()), "gate")
        claimed_fn = getattr(kh, stem + "_claimed")
        claimed_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(_ResultArrays), ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(Gate), ctypes.POINTER(ctypes.c_double)]
        rc = claimed_fn(flats[0]._h, ctypes.byref(ra), seq.ctypes.data if seq is not None else None, mask, ctypes.byref(out), ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return {"clean": out.n_findings == 0, "passes": {w: [_audit_totals(table_of[w], outs[w][i]) for i in range(n)] for w in names},
            "findings": table[:min(int(out.n_findings), cap_findings)].copy(), "n_findings": int(out.n_findings), "truncated": bool(out.truncated & KS_AUDIT_GATE_TRUNCATED),
            "ms": (float(ms[0]), float(ms[1]))}


def audit_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """Audit the results the last solve left on the device, for a whole batch in one launch sequence (include/kshost.h ksh_audit): handles of any kind whose results
    are there -- a Solve, what-ifs flattened one by one, what-ifs derived on the device.  One dict per problem, as `FlatProblem.audit` returns it."""
    return _audit("audit", flats)


def audit_topology_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's second pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_topology): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_topology` returns it."""
    return _audit("topology", flats)


def audit_spread_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's third pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_spread): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_spread` returns it."""
    return _audit("spread", flats)


def audit_firstfit_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's fourth pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_firstfit): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_firstfit` returns it."""
    return _audit("firstfit", flats)


def audit_limits_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's fifth pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_limits): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_limits` returns it."""
    return _audit("limits", flats)


def audit_hostfit_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's sixth pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_hostfit): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_hostfit` returns it."""
    return _audit("hostfit", flats)


def audit_zonefit_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's ninth pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_zonefit): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_zonefit` returns it."""
    return _audit("zonefit", flats)


def audit_stages_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's seventh pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_stages): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_stages` returns it."""
    return _audit("stages", flats)


def audit_reasons_batch(flats: Sequence["FlatProblem"]) -> List[dict]:
    """The audit's eighth pass over the results the last solve left on the device, for a whole batch (include/kshost.h ksh_audit_reasons): handles of any kind, derived
    what-ifs included.  One dict per problem, as `FlatProblem.audit_reasons` returns it."""
    return _audit("reasons", flats)


def deal_lpt(weights: Sequence[int], nshards: int) -> List[int]:
    """Which shard (GPU / rank) each what-if goes to: longest predicted work first, each to the least loaded shard (include/ksolve.h ks_deal_lpt) -- instead of i mod N, which
    leaves a batch as long as its longest what-if plus whatever happened to be dealt beside it."""
    n = len(weights)
    w = (ctypes.c_uint64 * max(1, n))(*[int(x) for x in weights])
    out = (ctypes.c_uint32 * max(1, n))()
    libs()[0].ks_deal_lpt(w, n, nshards, out)
    return [int(out[i]) for i in range(n)]


def solve_whatifs_sharded(shards: Sequence[Sequence[FlatProblem]], ids: Sequence[Sequence[int]], words: int):
    """The what-if fan-out in one C call (include/kshost.h ksh_solve_whatifs_sharded): every shard's what-ifs (resident on that shard's device) in one batched launch, all
    shards concurrently, the decision records gathered into one table ordered by id.  Returns ([n, 3 + words] uint64 numpy table, slowest shard's kernel milliseconds)."""
    import numpy as np
    kh = libs()[1]
    flat = [f for sh in shards for f in sh]
    n = len(flat)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flat])
    off = (ctypes.c_uint32 * (len(shards) + 1))(*([0] + list(np.cumsum([len(sh) for sh in shards]))))
    idv = (ctypes.c_uint64 * max(1, n))(*[int(i) for sh in ids for i in sh])
    rows = np.zeros((n, 3 + words), dtype=np.uint64)
    kms = ctypes.c_float()
    rc = kh.ksh_solve_whatifs_sharded(hs, off, len(shards), idv, words, rows.ctypes.data_as(ctypes.c_void_p), ctypes.byref(kms))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return rows, float(kms.value)


def result_records(flats: Sequence[FlatProblem], ids: Sequence[int], words: int):
    """[len(flats), 3 + words] int64 numpy table of fixed-size result records `[id, n_new, n_unscheduled, first new node's
    InstanceTypeOptions]` straight from the binary results (no text round trip): what the ranks exchange after a what-if batch."""
    import numpy as np
    kh = libs()[1]
    n = len(flats)
    rows = np.zeros((n, 2 + words), dtype=np.uint64)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    rc = kh.ksh_result_summaries(hs, n, rows.ctypes.data_as(ctypes.c_void_p), words)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    out = np.empty((n, 3 + words), dtype=np.uint64)
    out[:, 0] = np.asarray(ids, dtype=np.uint64)
    out[:, 1:] = rows
    return out.view(np.int64)


def solve_batch_resident(flats: Sequence[FlatProblem]):
    """The batched launch with the results left on the device (nothing but the error words is read back).  Returns (kernel ms, wall ms)."""
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    kms, wms = ctypes.c_float(), ctypes.c_double()
    rc = kh.ksh_solve_batch_resident(hs, n, ctypes.byref(kms), ctypes.byref(wms))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return float(kms.value), float(wms.value)


def result_records_dev(flats: Sequence[FlatProblem], ids: Sequence[int], words: int, out_tensor):
    """The records of `result_records`, built ON the device from the results a `solve_batch_resident` left there, into `out_tensor`: a contiguous
    int64 / uint64 device tensor [len(flats), 3 + words] on the problems' device (anything with .data_ptr()).  Complete on return."""
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    c_ids = (ctypes.c_uint64 * max(1, n))(*[int(x) for x in ids])
    rc = kh.ksh_result_records_dev(hs, n, c_ids, words, ctypes.c_void_p(int(out_tensor.data_ptr())))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return out_tensor


def upload_batch(flats: Sequence[FlatProblem], device: int = 0, threads: int = 0):
    """Upload a batch of problems (typically the what-ifs of one snapshot) on host threads."""
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    rc = kh.ksh_upload_batch(hs, n, device, threads)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())


def price_filter(flats: Sequence[FlatProblem], nodes: Sequence[int], max_prices: Sequence[float], spot_only: Optional[Sequence[bool]] = None) -> List[List[int]]:
    """filterByPrice (deprovisioning/helpers.go:148-157) on the device, over the results the last solve / solve_batch of
    `flats` left there: for flats[i], the instance-type indices of new node nodes[i]'s InstanceTypeOptions whose worst
    launch price is < max_prices[i] (ascending type index; the caller restores the option order).  spot_only[i]: price the
    node as if its capacity-type requirement were already In [spot] (consolidation.go:262-265)."""
    kh = libs()[1]
    n = len(flats)
    if n == 0:
        return []
    stride = max((f.dims["T"] + 63) // 64 for f in flats)
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    node = (ctypes.c_uint32 * n)(*[int(x) for x in nodes])
    mp = (ctypes.c_double * n)(*[float(x) for x in max_prices])
    masks = (ctypes.c_uint64 * (n * stride))()
    counts = (ctypes.c_uint32 * n)()
    so = (ctypes.c_uint32 * n)(*[1 if x else 0 for x in spot_only]) if spot_only is not None else None
    rc = kh.ksh_price_filter(hs, n, node, mp, so, masks, stride, counts)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    out = []
    for i in range(n):
        row = [w * 64 + b for w in range(stride) for b in range(64) if (masks[i * stride + w] >> b) & 1]
        assert len(row) == counts[i]
        out.append(row)
    return out


# ---- consolidation commands decided on the device (include/ksolve.h KS_CMD_*, include/kshost.h ksh_consolidation_commands) ----
KS_CMD_F_BLOCKED, KS_CMD_F_ALL_SPOT, KS_CMD_F_PRICE_ERROR, KS_CMD_F_SAME_TYPE = 1, 2, 4, 8
KS_CMD_ID, KS_CMD_DECISION, KS_CMD_N_NEW, KS_CMD_N_UNSCHEDULED, KS_CMD_N_OPTIONS, KS_CMD_N_OPTIONS_SAME_TYPE, KS_CMD_PRESENT, KS_CMD_IT_STATE = range(8)
KS_CMD_MASK, KS_CMD_BOUNDS, KS_CMD_OPTIONS = 8, 40, 72
KS_CMD_DO_NOTHING, KS_CMD_DELETE, KS_CMD_REPLACE, KS_CMD_ERROR = 0, 1, 2, 3
KS_CMD_WHY_NOT_ALL_SCHEDULED, KS_CMD_WHY_MANY_NODES, KS_CMD_WHY_PRICE_ERROR, KS_CMD_WHY_NOT_CHEAPER, KS_CMD_WHY_SPOT_TO_SPOT, KS_CMD_WHY_SAME_TYPE, KS_CMD_WHY_DELETING = 1, 3, 4, 6, 7, 9, 10
COMMAND_TIMING_KEYS = ("open_ms", "solve_ms", "command_kernel_ms", "readback_ms", "host_ms")


def command_row_words(words: int) -> int:
    """KS_CMD_ROW_WORDS: uint64 words of one command row whose option masks are `words` wide."""
    return KS_CMD_OPTIONS + 2 * words


class _CommandInputs(ctypes.Structure):      # include/ksolve.h ks_command_inputs
    _fields_ = [("flags", ctypes.c_void_p), ("cand_price", ctypes.c_void_p), ("type_off", ctypes.c_void_p), ("type_idx", ctypes.c_void_p), ("type_price", ctypes.c_void_p)]


def _u32s(xs):
    import numpy as np
    a = np.ascontiguousarray(np.asarray(list(xs), dtype=np.uint32))
    return a if a.size else np.zeros(1, dtype=np.uint32)


def _cand_csr(candidate_sets):
    import numpy as np
    off = np.zeros(len(candidate_sets) + 1, dtype=np.uint32)
    np.cumsum([len(cs) for cs in candidate_sets], out=off[1:])
    return off, _u32s(c for cs in candidate_sets for c in cs)


def _pod_node_arg(pod_node):
    import numpy as np
    if pod_node is None:
        return None, None
    pn = np.ascontiguousarray(np.asarray(pod_node, dtype=np.int32)) if len(pod_node) else np.zeros(1, dtype=np.int32)
    return pn, pn.ctypes.data


def consolidation_commands(snapshot: "ParsedProblem", pod_node: Optional[Sequence[int]], candidate_sets: Sequence[Sequence[int]], words: int, deleting: Sequence[int] = (),
                           same_type: bool = False, device: int = 0, volumes: bool = False, active_resources: bool = False, flags: int = 0):
    """computeConsolidation for every candidate set in ONE call (kshost.h `ksh_consolidation_commands`): what-ifs derived, solved resident and decided on the
    device; only the fixed-size rows come back.  Returns (numpy uint64 [n, command_row_words(words)], {open_ms, solve_ms, command_kernel_ms, readback_ms, host_ms}: the library's own split of the call)."""
    import numpy as np
    kh = libs()[1]
    n = len(candidate_sets)
    off, cand = _cand_csr(candidate_sets)
    pn, pn_ptr = _pod_node_arg(pod_node)
    dl = _u32s(deleting)
    rows = np.zeros((max(1, n), command_row_words(words)), dtype=np.uint64)
    ms = (ctypes.c_double * 5)()
    kh.ksh_consolidation_commands.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]
    rc = kh.ksh_consolidation_commands(snapshot._p, (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags, n, off.ctypes.data, cand.ctypes.data,
                                       pn_ptr, dl.ctypes.data, len(deleting), device, 1 if same_type else 0, rows.ctypes.data, words, ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return rows[:n], dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms]))


def _search_option(name: str, snapshot, pod_node, candidates, words, deleting, device, volumes, active_resources, flags, max_nodes=None):
    import numpy as np
    kh = libs()[1]
    cand, dl = _u32s(candidates), _u32s(deleting)
    pn, pn_ptr = _pod_node_arg(pod_node)
    row = np.zeros(command_row_words(words), dtype=np.uint64)
    ms = (ctypes.c_double * 5)()
    fl = (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags
    fn = getattr(kh, name)
    head = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    tail = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]
    if max_nodes is None:
        fn.argtypes = head + tail
        rc = fn(snapshot._p, fl, cand.ctypes.data, len(candidates), pn_ptr, dl.ctypes.data, len(deleting), device, row.ctypes.data, words, ms)
    else:
        fn.argtypes = head + [ctypes.c_uint32] + tail
        rc = fn(snapshot._p, fl, cand.ctypes.data, len(candidates), max_nodes, pn_ptr, dl.ctypes.data, len(deleting), device, row.ctypes.data, words, ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return row, dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms]))


def first_n_node_option(snapshot: "ParsedProblem", pod_node, candidates: Sequence[int], words: int, max_nodes: int = 100, deleting: Sequence[int] = (), device: int = 0,
                        volumes: bool = False, active_resources: bool = False, flags: int = 0):
    """firstNNodeConsolidationOption (kshost.h `ksh_first_n_node_option`): every prefix in one batch, the binary search replayed over the rows.  Returns (row, timings);
    row[KS_CMD_ID] = how many leading candidates the command removes."""
    return _search_option("ksh_first_n_node_option", snapshot, pod_node, candidates, words, deleting, device, volumes, active_resources, flags, max_nodes=max_nodes)


def single_node_option(snapshot: "ParsedProblem", pod_node, candidates: Sequence[int], words: int, deleting: Sequence[int] = (), device: int = 0,
                       volumes: bool = False, active_resources: bool = False, flags: int = 0):
    """The scan of SingleNodeConsolidation.ComputeCommand (kshost.h `ksh_single_node_option`).  Returns (row, timings); row[KS_CMD_ID] = the candidate's position."""
    return _search_option("ksh_single_node_option", snapshot, pod_node, candidates, words, deleting, device, volumes, active_resources, flags)


# ---- consolidation commands validated on the device (include/ksolve.h KS_VAL_*, include/kshost.h ksh_validate_commands) ----
KS_VAL_F_BLOCKED, KS_VAL_F_EXPECT_REPLACEMENT = 1, 2
KS_VAL_ID, KS_VAL_VERDICT, KS_VAL_N_NEW, KS_VAL_N_UNSCHEDULED, KS_VAL_N_MAPPED, KS_VAL_N_OPTIONS, KS_VAL_N_MISSING = range(7)
KS_VAL_OPTIONS = 8
KS_VAL_INVALID, KS_VAL_VALID, KS_VAL_ERROR = 0, 1, 2
(KS_VAL_WHY_VALID, KS_VAL_WHY_NOMINATED, KS_VAL_WHY_NO_CANDIDATES, KS_VAL_WHY_DELETING, KS_VAL_WHY_NOT_ALL_SCHEDULED, KS_VAL_WHY_NO_NEW_NODE, KS_VAL_WHY_MANY_NODES,
 KS_VAL_WHY_UNEXPECTED_NODE, KS_VAL_WHY_NOT_A_SUBSET) = range(9)


def validation_row_words(words: int) -> int:
    """KS_VAL_ROW_WORDS: uint64 words of one validation row whose option masks are `words` wide."""
    return KS_VAL_OPTIONS + 2 * words


def _type_masks(type_sets, words):
    import numpy as np
    m = np.zeros((max(1, len(type_sets)), words), dtype=np.uint64)
    for i, ts in enumerate(type_sets):
        for t in ts:
            m[i, t // 64] |= np.uint64(1 << (t % 64))
    return m


def validate_commands(snapshot: "ParsedProblem", pod_node: Optional[Sequence[int]], node_sets: Sequence[Sequence[int]], expect_replacement: Sequence[bool],
                      type_sets: Sequence[Sequence[int]], why: Sequence[int], node_flags: Sequence[int], words: int, deleting: Sequence[int] = (), device: int = 0,
                      volumes: bool = False, active_resources: bool = False, flags: int = 0, out=None, node_off=None, options=None):
    """Validation.IsValid / ValidateCommand for every command in ONE call (kshost.h `ksh_validate_commands`) over the snapshot as it is now: node_sets[i] = the command's
    nodesToRemove as node slots, type_sets[i] = its replacement's instance-type indices (read where expect_replacement[i]), why / node_flags per node slot
    (`consolidation_candidates`' why over this snapshot; KSH_CAND_NODE_NOMINATED is read).  Returns (numpy uint64 [n, validation_row_words(words)], the library's split
    of the call).  `out`: a preallocated array to fill; `node_off` / `options`: raw arrays to pass instead (tests: malformed input)."""
    import numpy as np
    kh = libs()[1]
    n = len(node_sets)
    off, nodes = _cand_csr(node_sets)
    if node_off is not None:
        off = _u32s(node_off)
    ex = _u32s(1 if e else 0 for e in expect_replacement)
    opts = np.ascontiguousarray(options) if options is not None else _type_masks(type_sets, words)
    wy, nf = _u32s(why), _u32s(node_flags)
    pn, pn_ptr = _pod_node_arg(pod_node)
    dl = _u32s(deleting)
    rows = out if out is not None else np.zeros((max(1, n), validation_row_words(words)), dtype=np.uint64)
    ms = (ctypes.c_double * 5)()
    kh.ksh_validate_commands.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + [ctypes.c_void_p] * 7 + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p,
                                                                                                                       ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]
    rc = kh.ksh_validate_commands(snapshot._p, (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags, n, off.ctypes.data, nodes.ctypes.data,
                                  ex.ctypes.data, opts.ctypes.data, wy.ctypes.data, nf.ctypes.data, pn_ptr, dl.ctypes.data, len(deleting), device, rows.ctypes.data, words, ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return rows[:n], dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms]))


def decode_validation_row(row, words: int) -> dict:
    """A validation row as Python values: verdict (True / False / None for the error), why, counts, the re-simulation's options and the command's missing types as indices."""
    r = [int(x) for x in row]
    bits = lambda base: [w * 64 + b for w in range(words) for b in range(64) if (r[base + w] >> b) & 1]
    verdict = r[KS_VAL_VERDICT] & 0xFF
    return {"id": r[KS_VAL_ID], "valid": None if verdict == KS_VAL_ERROR else verdict == KS_VAL_VALID, "why": (r[KS_VAL_VERDICT] >> 8) & 0xFF, "n_new": r[KS_VAL_N_NEW],
            "n_unscheduled": r[KS_VAL_N_UNSCHEDULED], "n_mapped": r[KS_VAL_N_MAPPED], "n_options": r[KS_VAL_N_OPTIONS], "n_missing": r[KS_VAL_N_MISSING], "reserved": r[7],
            "options": bits(KS_VAL_OPTIONS), "missing": bits(KS_VAL_OPTIONS + words)}


def single_node_resume(snapshot: "ParsedProblem", pod_node, candidates: Sequence[int], failed_before: bool, why: Sequence[int], node_flags: Sequence[int], words: int,
                       deleting: Sequence[int] = (), device: int = 0, volumes: bool = False, active_resources: bool = False, flags: int = 0):
    """The rest of SingleNodeConsolidation.ComputeCommand's loop after a failed validation (kshost.h `ksh_single_node_resume`).  Returns (state: 1 found / 2 retry /
    0 do-nothing, command row, validation row, timings); row[KS_CMD_ID] = the found candidate's position."""
    import numpy as np
    kh = libs()[1]
    cand, dl, wy, nf = _u32s(candidates), _u32s(deleting), _u32s(why), _u32s(node_flags)
    pn, pn_ptr = _pod_node_arg(pod_node)
    row, vrow = np.zeros(command_row_words(words), dtype=np.uint64), np.zeros(validation_row_words(words), dtype=np.uint64)
    state, ms = ctypes.c_uint32(99), (ctypes.c_double * 5)()
    kh.ksh_single_node_resume.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]
    rc = kh.ksh_single_node_resume(snapshot._p, (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags, cand.ctypes.data, len(candidates),
                                   1 if failed_before else 0, wy.ctypes.data, nf.ctypes.data, pn_ptr, dl.ctypes.data, len(deleting), device, row.ctypes.data, vrow.ctypes.data,
                                   ctypes.byref(state), words, ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return int(state.value), row, vrow, dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms]))


def validate_empty_nodes(nodes: Sequence[int], why: Sequence[int], n_node_pods: Sequence[int], node_flags: Sequence[int]) -> bool:
    """EmptyNodeConsolidation's own check (kshost.h `ksh_validate_empty_nodes`, host only): True = retry."""
    kh = libs()[1]
    nd, wy, npods, nf = _u32s(nodes), _u32s(why), _u32s(n_node_pods), _u32s(node_flags)
    retry = ctypes.c_uint32(99)
    kh.ksh_validate_empty_nodes.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    rc = kh.ksh_validate_empty_nodes(nd.ctypes.data, len(nodes), wy.ctypes.data, npods.ctypes.data, nf.ctypes.data, ctypes.byref(retry))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return bool(retry.value)


KSH_CAND_NODE_NOMINATED, KSH_CAND_NODE_DO_NOT_CONSOLIDATE, KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE, KSH_CAND_NODE_DELETION_TIMESTAMP = 1, 2, 4, 8      # kshost.h
KSH_CAND_POD_DO_NOT_EVICT, KSH_CAND_POD_HAS_DELETION_COST, KSH_CAND_POD_HAS_PRIORITY = 1, 2, 4
KS_CAND_MAX_KEYS, KS_CAND_MAX_VALUES = 16, 62
KSH_CAND_WIDE_SELECTORS = 1      # kshost.h: the `flags` bit of ksh_*_candidates_ex
CANDIDATE_TIMING_KEYS = ("host_ms", "upload_ms", "kernels_ms", "readback_ms")


class _CandidateInputs(ctypes.Structure):      # include/kshost.h ksh_candidate_inputs
    _fields_ = [("n_nodes", ctypes.c_uint32), ("n_pods", ctypes.c_uint32), ("n_provisioners", ctypes.c_uint32), ("pad", ctypes.c_uint32), ("node_flags", ctypes.c_void_p),
                ("node_age_seconds", ctypes.c_void_p), ("pod_flags", ctypes.c_void_p), ("pod_deletion_cost", ctypes.c_void_p), ("pod_priority", ctypes.c_void_p),
                ("prov_consolidation_enabled", ctypes.c_void_p), ("prov_ttl_seconds_until_expired", ctypes.c_void_p)]


class _PdbBlock(ctypes.Structure):      # include/kshost.h ksh_pdb_block
    _fields_ = [("n_pdbs", ctypes.c_uint32), ("n_strings", ctypes.c_uint32), ("n_words", ctypes.c_uint32), ("str_off", ctypes.c_void_p), ("str_bytes", ctypes.c_void_p),
                ("words", ctypes.c_void_p), ("str_bytes_len", ctypes.c_uint64)]


class _CandidatesOut(ctypes.Structure):      # include/kshost.h ksh_candidates_out
    _fields_ = [("n_candidates", ctypes.c_uint32), ("n_empty", ctypes.c_uint32), ("order", ctypes.c_void_p), ("empty", ctypes.c_void_p), ("why", ctypes.c_void_p),
                ("detail", ctypes.c_void_p), ("n_node_pods", ctypes.c_void_p), ("cost", ctypes.c_void_p)]


def consolidation_candidates(snapshot: "ParsedProblem", pod_node: Optional[Sequence[int]], node_flags: Sequence[int], node_age_seconds: Sequence[float],
                             pod_flags: Sequence[int], pod_deletion_cost: Sequence[float], pod_priority: Sequence[int], prov_consolidation_enabled: Sequence[bool],
                             prov_ttl_seconds: Sequence[Optional[int]], pdbs=(), deleting: Sequence[int] = (), device: int = 0, out: Optional[dict] = None,
                             wide_selectors: bool = False) -> dict:
    """candidateNodes + consolidation.ShouldDeprovision + sortAndFilterCandidates in ONE call (kshost.h `ksh_consolidation_candidates_ex`): the per-pod eviction costs and
    PDB matches, the per-node sums and reasons and the order are computed on the device.  The arrays run over the snapshot's node / pod slots and its provisioners;
    `pdbs`: `model.PodDisruptionBudget`s, or the block `model.pdbs_to_block` made of them; `prov_ttl_seconds`: None (or -1) for nil.  Returns {"order", "empty": lists of
    node slots; "why", "detail", "n_node_pods": int arrays per node slot; "cost": float64 per node slot; "ms": the library's split of the call}.  `order` is what
    `first_n_node_option` / `single_node_option` take as candidates.  `out`: preallocated arrays to fill instead
    ({"order", "empty", "why", "n_node_pods": uint32, "detail": int32, "cost": float64}, one entry per node slot).  `wide_selectors`: KSH_CAND_WIDE_SELECTORS -- the
    selectors go to the device as lists, so label keys, values per key and set sizes are unbounded (without it more than 16 keys or 62 values of a key are refused)."""
    import numpy as np
    from .model import pdbs_to_block
    kh = libs()[1]
    nf = np.ascontiguousarray(np.asarray(list(node_flags) or [0], dtype=np.uint32)); age = np.ascontiguousarray(np.asarray(list(node_age_seconds) or [0.0], dtype=np.float64))
    pf = np.ascontiguousarray(np.asarray(list(pod_flags) or [0], dtype=np.uint32)); dc = np.ascontiguousarray(np.asarray(list(pod_deletion_cost) or [0.0], dtype=np.float64))
    pp = np.ascontiguousarray(np.asarray(list(pod_priority) or [0], dtype=np.int32))
    en = np.ascontiguousarray(np.asarray([1 if e else 0 for e in prov_consolidation_enabled] or [0], dtype=np.uint32))
    ttl = np.ascontiguousarray(np.asarray([-1 if t is None else int(t) for t in prov_ttl_seconds] or [-1], dtype=np.int64))
    n_nodes, n_pods = len(node_flags), len(pod_flags)
    if len(node_age_seconds) != n_nodes or len(pod_deletion_cost) != n_pods or len(pod_priority) != n_pods or len(prov_ttl_seconds) != len(prov_consolidation_enabled):
        raise KSolveError(KS_ERR_INVALID, "consolidation_candidates: array lengths differ")
    inp = _CandidateInputs(n_nodes, n_pods, len(prov_consolidation_enabled), 0, nf.ctypes.data, age.ctypes.data, pf.ctypes.data, dc.ctypes.data, pp.ctypes.data, en.ctypes.data, ttl.ctypes.data)
    b = pdbs if isinstance(pdbs, dict) else pdbs_to_block(list(pdbs))
    pb = _PdbBlock(b["n_pdbs"], b["n_strings"], b["n_words"], b["str_off"].ctypes.data, b["str_bytes"].ctypes.data, b["words"].ctypes.data, int(b.get("str_bytes_len", b["str_bytes"].size)))
    m = max(1, n_nodes)
    if out is not None:          # (tests: preallocated arrays, poisoned first)
        order, empty, why, npods, detail, cost = (out[k] for k in ("order", "empty", "why", "n_node_pods", "detail", "cost"))
    else:
        order, empty, why, npods = (np.zeros(m, dtype=np.uint32) for _ in range(4))
        detail, cost = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.float64)
    out = _CandidatesOut(0, 0, order.ctypes.data, empty.ctypes.data, why.ctypes.data, detail.ctypes.data, npods.ctypes.data, cost.ctypes.data)
    pn, pn_ptr = _pod_node_arg(pod_node)
    dl = _u32s(deleting)
    ms = (ctypes.c_double * 4)()
    kh.ksh_consolidation_candidates_ex.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                                   ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    rc = kh.ksh_consolidation_candidates_ex(snapshot._p, pn_ptr, dl.ctypes.data, len(deleting), ctypes.byref(inp), ctypes.byref(pb), device,
                                            KSH_CAND_WIDE_SELECTORS if wide_selectors else 0, ctypes.byref(out), ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return {"order": [int(x) for x in order[:out.n_candidates]], "empty": [int(x) for x in empty[:out.n_empty]], "why": why[:n_nodes], "detail": detail[:n_nodes],
            "n_node_pods": npods[:n_nodes], "cost": cost[:n_nodes], "ms": dict(zip(CANDIDATE_TIMING_KEYS, [float(x) for x in ms]))}


# ---- candidates of expiration / drift / emptiness (include/kshost.h ksh_deprovisioning_candidates, ksh_emptiness_command) ----
KSH_METHOD_EXPIRATION, KSH_METHOD_DRIFT, KSH_METHOD_EMPTINESS = 1, 2, 3
KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP, KSH_CAND_NODE_EMPTINESS_UNPARSABLE, KSH_CAND_NODE_DRIFTED = 16, 32, 64
KS_DEPROV_WHY_NOT_EXPIRED, KS_DEPROV_WHY_NOT_DRIFTED, KS_DEPROV_WHY_NOT_EMPTY = 14, 15, 16
KS_DEPROV_MAX_TTL_SECONDS = 9223372036


class _DeprovisioningInputs(ctypes.Structure):      # include/kshost.h ksh_deprovisioning_inputs
    _fields_ = [("base", _CandidateInputs), ("now_unix_nanos", ctypes.c_int64), ("node_creation_unix_nanos", ctypes.c_void_p), ("node_emptiness_unix_nanos", ctypes.c_void_p),
                ("prov_ttl_seconds_after_empty", ctypes.c_void_p), ("drift_enabled", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


class _DeprovisioningOut(ctypes.Structure):      # include/kshost.h ksh_deprovisioning_out
    _fields_ = [("base", _CandidatesOut), ("n_in_result", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


def deprovisioning_candidates(snapshot: "ParsedProblem", method: int, pod_node: Optional[Sequence[int]], now_unix_nanos: int, node_flags: Sequence[int],
                              node_creation_unix_nanos: Sequence[int], node_age_seconds: Sequence[float], pod_flags: Sequence[int], pod_deletion_cost: Sequence[float],
                              pod_priority: Sequence[int], prov_ttl_seconds: Sequence[Optional[int]], prov_ttl_seconds_after_empty: Sequence[Optional[int]] = None,
                              node_emptiness_unix_nanos: Sequence[int] = None, drift_enabled: bool = False, pdbs=(), deleting: Sequence[int] = (), device: int = 0,
                              out: Optional[dict] = None, wide_selectors: bool = False) -> dict:
    """candidateNodes under Expiration / Drift / Emptiness.ShouldDeprovision and the order their ComputeCommand walks, in ONE call (kshost.h
    `ksh_deprovisioning_candidates_ex`; `method`: KSH_METHOD_*; `wide_selectors`: as for `consolidation_candidates`).  Arrays as for `consolidation_candidates`; times are unix nanoseconds as Python ints (exact int64 arithmetic
    on the device); `node_flags` may carry KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP / _EMPTINESS_UNPARSABLE / _DRIFTED; ttls: None (or -1) for nil.  Returns
    `consolidation_candidates`' dict plus "n_in_result": len(candidateNodes(...)) -- the controller moves to the next method when it is 0."""
    import numpy as np
    from .model import pdbs_to_block
    kh = libs()[1]
    n_nodes, n_pods, n_prov = len(node_flags), len(pod_flags), len(prov_ttl_seconds)
    if prov_ttl_seconds_after_empty is None:
        prov_ttl_seconds_after_empty = [None] * n_prov
    if node_emptiness_unix_nanos is None:
        node_emptiness_unix_nanos = [0] * n_nodes
    if (len(node_age_seconds) != n_nodes or len(node_creation_unix_nanos) != n_nodes or len(node_emptiness_unix_nanos) != n_nodes or len(pod_deletion_cost) != n_pods or
            len(pod_priority) != n_pods or len(prov_ttl_seconds_after_empty) != n_prov):
        raise KSolveError(KS_ERR_INVALID, "deprovisioning_candidates: array lengths differ")
    i64 = lambda xs, fill: np.ascontiguousarray(np.asarray([fill if x is None else int(x) for x in xs] or [fill], dtype=np.int64))
    nf = np.ascontiguousarray(np.asarray(list(node_flags) or [0], dtype=np.uint32)); age = np.ascontiguousarray(np.asarray(list(node_age_seconds) or [0.0], dtype=np.float64))
    pf = np.ascontiguousarray(np.asarray(list(pod_flags) or [0], dtype=np.uint32)); dc = np.ascontiguousarray(np.asarray(list(pod_deletion_cost) or [0.0], dtype=np.float64))
    pp = np.ascontiguousarray(np.asarray(list(pod_priority) or [0], dtype=np.int32))
    ttl, ttl_e, cre, emp = i64(prov_ttl_seconds, -1), i64(prov_ttl_seconds_after_empty, -1), i64(node_creation_unix_nanos, 0), i64(node_emptiness_unix_nanos, 0)
    base = _CandidateInputs(n_nodes, n_pods, n_prov, 0, nf.ctypes.data, age.ctypes.data, pf.ctypes.data, dc.ctypes.data, pp.ctypes.data, None, ttl.ctypes.data)
    inp = _DeprovisioningInputs(base, int(now_unix_nanos), cre.ctypes.data, emp.ctypes.data, ttl_e.ctypes.data, 1 if drift_enabled else 0, 0)
    b = pdbs if isinstance(pdbs, dict) else pdbs_to_block(list(pdbs))
    pb = _PdbBlock(b["n_pdbs"], b["n_strings"], b["n_words"], b["str_off"].ctypes.data, b["str_bytes"].ctypes.data, b["words"].ctypes.data, int(b.get("str_bytes_len", b["str_bytes"].size)))
    m = max(1, n_nodes)
    if out is not None:          # (tests: preallocated arrays, poisoned first)
        order, empty, why, npods, detail, cost = (out[k] for k in ("order", "empty", "why", "n_node_pods", "detail", "cost"))
    else:
        order, empty, why, npods = (np.zeros(m, dtype=np.uint32) for _ in range(4))
        detail, cost = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.float64)
    res = _DeprovisioningOut(_CandidatesOut(0, 0, order.ctypes.data, empty.ctypes.data, why.ctypes.data, detail.ctypes.data, npods.ctypes.data, cost.ctypes.data), 0, 0)
    pn, pn_ptr = _pod_node_arg(pod_node)
    dl = _u32s(deleting)
    ms = (ctypes.c_double * 4)()
    kh.ksh_deprovisioning_candidates_ex.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                                    ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    rc = kh.ksh_deprovisioning_candidates_ex(snapshot._p, method, pn_ptr, dl.ctypes.data, len(deleting), ctypes.byref(inp), ctypes.byref(pb), device,
                                             KSH_CAND_WIDE_SELECTORS if wide_selectors else 0, ctypes.byref(res), ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return {"order": [int(x) for x in order[:res.base.n_candidates]], "empty": [int(x) for x in empty[:res.base.n_empty]], "why": why[:n_nodes], "detail": detail[:n_nodes],
            "n_node_pods": npods[:n_nodes], "cost": cost[:n_nodes], "n_in_result": int(res.n_in_result), "ms": dict(zip(CANDIDATE_TIMING_KEYS, [float(x) for x in ms]))}


def emptiness_command(candidates: Sequence[int], n_node_pods: Sequence[int]):
    """Emptiness.ComputeCommand (kshost.h `ksh_emptiness_command`, host only) over `deprovisioning_candidates`' order and n_node_pods under KSH_METHOD_EMPTINESS:
    (KS_CMD_DELETE or KS_CMD_DO_NOTHING, the node slots to remove)."""
    import numpy as np
    kh = libs()[1]
    cand, npods = _u32s(candidates), _u32s(n_node_pods)
    nodes = np.zeros(max(1, len(candidates)), dtype=np.uint32)
    action, n = ctypes.c_uint32(99), ctypes.c_uint32(0)
    kh.ksh_emptiness_command.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    rc = kh.ksh_emptiness_command(cand.ctypes.data, len(candidates), npods.ctypes.data, ctypes.byref(action), nodes.ctypes.data, ctypes.byref(n))
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return int(action.value), [int(x) for x in nodes[:n.value]]


# ---- replacement commands with m -> n rows (include/ksolve.h KS_REP_*, include/kshost.h ksh_replacement_commands / ksh_replacement_option / ksh_replacement_rows) ----
KS_REP_F_BLOCKED = 1
KS_REP_HEAD_WORDS = 8
KS_REP_ID, KS_REP_DECISION, KS_REP_N_NEW, KS_REP_N_UNSCHEDULED, KS_REP_N_NODES, KS_REP_NODE_OFF, KS_REP_N_OPTIONS = range(7)
KS_REP_BLOCKED, KS_REP_TRUNCATED = 1, 2
KS_REP_NODE_ID, KS_REP_NODE_PRESENT, KS_REP_NODE_IT_STATE, KS_REP_NODE_N_OPTIONS, KS_REP_NODE_REQMASK, KS_REP_NODE_MASK, KS_REP_NODE_BOUNDS, KS_REP_NODE_REQ, KS_REP_NODE_OPTIONS = 0, 1, 2, 3, 4, 5, 37, 69, 85
KS_MAX_RES = 16


def replacement_node_words(words: int) -> int:
    """KS_REP_NODE_WORDS: uint64 words of one node row whose option mask is `words` wide."""
    return KS_REP_NODE_OPTIONS + words


def _rep_tables(n, cap_nodes, words, heads, nodes):
    import numpy as np
    if heads is None:
        heads = np.zeros((max(1, n), KS_REP_HEAD_WORDS), dtype=np.uint64)
    if nodes is None and cap_nodes:
        nodes = np.zeros((cap_nodes, replacement_node_words(words)), dtype=np.uint64)
    return heads, nodes


def replacement_commands(snapshot: "ParsedProblem", pod_node: Optional[Sequence[int]], candidate_sets: Sequence[Sequence[int]], words: int, cap_nodes: Optional[int] = None,
                         deleting: Sequence[int] = (), device: int = 0, volumes: bool = False, active_resources: bool = False, flags: int = 0, heads=None, nodes=None):
    """Expiration / Drift.ComputeCommand's simulation and m -> n command for every candidate set in ONE call (kshost.h `ksh_replacement_commands`).  cap_nodes None:
    the sizing call first, then a table that is exactly large enough.  `heads` / `nodes`: preallocated tables to fill (tests poison them; their row widths must be
    KS_REP_HEAD_WORDS / replacement_node_words(words)).  Returns (heads [n, 8], nodes [cap_nodes, replacement_node_words(words)] or None, total nodes, timings)."""
    kh = libs()[1]
    n = len(candidate_sets)
    off, cand = _cand_csr(candidate_sets)
    pn, pn_ptr = _pod_node_arg(pod_node)
    dl = _u32s(deleting)
    fl = (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags
    kh.ksh_replacement_commands.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_uint32, ctypes.POINTER(ctypes.c_double)]

    def call(cap, hd, nd):
        total, ms = ctypes.c_uint64(0), (ctypes.c_double * 5)()
        rc = kh.ksh_replacement_commands(snapshot._p, fl, n, off.ctypes.data, cand.ctypes.data, pn_ptr, dl.ctypes.data, len(deleting), device, hd.ctypes.data,
                                         nd.ctypes.data if nd is not None else None, cap, ctypes.byref(total), words, ms)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return int(total.value), dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms]))
    if cap_nodes is None:
        hd, _ = _rep_tables(n, 0, words, None, None)
        cap_nodes, _ = call(0, hd, None)
    heads, nodes = _rep_tables(n, cap_nodes, words, heads, nodes)
    total, ms = call(cap_nodes, heads, nodes)
    return heads[:n], nodes, total, ms


def replacement_option(snapshot: "ParsedProblem", pod_node, candidates: Sequence[int], why: Sequence[int], words: int, cap_nodes: int = 64, deleting: Sequence[int] = (), device: int = 0,
                       volumes: bool = False, active_resources: bool = False, flags: int = 0):
    """ComputeCommand's loop for expiration and drift (kshost.h `ksh_replacement_option`): the first candidate with why == 0 that is not deleting is simulated, alone.
    Returns (head, nodes, total nodes, position in `candidates` or -1, timings); called again with a larger table if `cap_nodes` was too small."""
    import numpy as np
    kh = libs()[1]
    cand, wy, dl = _u32s(candidates), _u32s(why), _u32s(deleting)
    pn, pn_ptr = _pod_node_arg(pod_node)
    fl = (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags
    kh.ksh_replacement_option.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32), ctypes.c_uint32,
                                          ctypes.POINTER(ctypes.c_double)]
    while True:
        head = np.zeros(KS_REP_HEAD_WORDS, dtype=np.uint64)
        nodes = np.zeros((max(1, cap_nodes), replacement_node_words(words)), dtype=np.uint64)
        total, pos, ms = ctypes.c_uint64(0), ctypes.c_int32(-2), (ctypes.c_double * 5)()
        rc = kh.ksh_replacement_option(snapshot._p, fl, cand.ctypes.data, len(candidates), wy.ctypes.data, pn_ptr, dl.ctypes.data, len(deleting), device, head.ctypes.data, nodes.ctypes.data,
                                       cap_nodes, ctypes.byref(total), ctypes.byref(pos), words, ms)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        if int(total.value) <= cap_nodes:
            return head, nodes[:int(total.value)], int(total.value), int(pos.value), dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms]))
        cap_nodes = int(total.value)


def whatifs_simulated() -> int:
    """`ksh_whatifs_simulated`: what-ifs the simulating calls have opened and solved in this process so far; the difference across a call counts its simulations."""
    kh = libs()[1]
    kh.ksh_whatifs_simulated.restype = ctypes.c_uint64
    kh.ksh_whatifs_simulated.argtypes = []
    return int(kh.ksh_whatifs_simulated())


def replacement_rows(flats: Sequence[FlatProblem], ids: Sequence[int], flags: Sequence[int], words: int, cap_nodes: int, heads=None, nodes=None):
    """`ksh_replacement_rows`: both tables of handles whose results are on the device.  Returns (heads, nodes or None, total nodes)."""
    import numpy as np
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    c_ids = np.ascontiguousarray(np.asarray(list(ids) or [0], dtype=np.uint64))
    fl = _u32s(flags)
    heads, nodes = _rep_tables(n, cap_nodes, words, heads, nodes)
    total = ctypes.c_uint64(0)
    kh.ksh_replacement_rows.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    rc = kh.ksh_replacement_rows(hs, n, c_ids.ctypes.data, fl.ctypes.data, words, heads.ctypes.data, nodes.ctypes.data if nodes is not None else None, cap_nodes, ctypes.byref(total), None)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return heads[:n], nodes, int(total.value)


def decode_replacement_head(head) -> dict:
    r = [int(x) for x in head]
    return {"id": r[KS_REP_ID], "action": r[KS_REP_DECISION] & 0xFF, "why": (r[KS_REP_DECISION] >> 8) & 0xFF, "blocked": bool((r[KS_REP_DECISION] >> 16) & KS_REP_BLOCKED),
            "truncated": bool((r[KS_REP_DECISION] >> 16) & KS_REP_TRUNCATED), "n_new": r[KS_REP_N_NEW], "n_unscheduled": r[KS_REP_N_UNSCHEDULED], "n_nodes": r[KS_REP_N_NODES],
            "node_off": r[KS_REP_NODE_OFF], "n_options": r[KS_REP_N_OPTIONS], "reserved": r[7]}


def decode_replacement_node(snapshot: "ParsedProblem", row, words: int) -> dict:
    """A node row as Python values, through the handle-free name accessors: what-if id, node index, options as instance-type indices, requirements as
    `decode_command_row` gives them, requests {resource name: milli-units} for the resources the request mask lists."""
    kh = libs()[1]
    r = [int(x) for x in row]
    as_cmd = [0] * command_row_words(words)      # the requirement words have KS_CMD_*'s layout and meaning: decoded by the same code
    as_cmd[KS_CMD_PRESENT], as_cmd[KS_CMD_IT_STATE] = r[KS_REP_NODE_PRESENT], r[KS_REP_NODE_IT_STATE]
    as_cmd[KS_CMD_MASK:KS_CMD_MASK + 32] = r[KS_REP_NODE_MASK:KS_REP_NODE_MASK + 32]
    as_cmd[KS_CMD_BOUNDS:KS_CMD_BOUNDS + 32] = r[KS_REP_NODE_BOUNDS:KS_REP_NODE_BOUNDS + 32]
    reqs = decode_command_row(snapshot, as_cmd, words)["requirements"]
    kh.ksh_snapshot_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
    kh.ksh_snapshot_name.restype = ctypes.c_char_p
    requests = {}
    for a in range(KS_MAX_RES):
        if (r[KS_REP_NODE_REQMASK] >> a) & 1:
            v = r[KS_REP_NODE_REQ + a]
            requests[kh.ksh_snapshot_name(snapshot._p, 2, a, 0).decode()] = v - (1 << 64) if v >= (1 << 63) else v
    return {"id": r[KS_REP_NODE_ID] & 0xFFFFFFFF, "node": r[KS_REP_NODE_ID] >> 32, "n_options": r[KS_REP_NODE_N_OPTIONS], "reqmask": r[KS_REP_NODE_REQMASK],
            "options": [w * 64 + b for w in range(words) for b in range(64) if (r[KS_REP_NODE_OPTIONS + w] >> b) & 1], "requirements": reqs, "requests": requests,
            "req_words": r[KS_REP_NODE_REQ:KS_REP_NODE_REQ + KS_MAX_RES]}


# ---- placement rows and provisioning over the snapshot (include/ksolve.h KS_PLC_*, include/kshost.h ksh_provision / ksh_placement_rows) ----
KS_PLC_HEAD_WORDS, KS_PLC_ROW_WORDS = 8, 4
KS_PLC_ID, KS_PLC_P, KS_PLC_N_NEW, KS_PLC_N_UNSCHEDULED, KS_PLC_ROW_OFF, KS_PLC_FLAGS, KS_PLC_N_EXISTING = range(7)
KS_PLC_POD_WHERE, KS_PLC_STAGE_SEQ, KS_PLC_REASON_ID, KS_PLC_POSITION = range(4)
KS_PLC_TRUNCATED, KSH_PROVISION_MACHINES_TRUNCATED = 1, 2
KSH_PROVISION_NOTHING, KSH_PROVISION_DERIVED, KSH_PROVISION_FLATTENED = 0, 1, 2
PROVISION_ROUTES = {KSH_PROVISION_NOTHING: "nothing", KSH_PROVISION_DERIVED: "derived", KSH_PROVISION_FLATTENED: "flattened"}


class _ProvisionOut(ctypes.Structure):      # include/kshost.h ksh_provision_out
    _fields_ = [("words", ctypes.c_uint32), ("route", ctypes.c_uint32), ("cap_rows", ctypes.c_uint64), ("cap_machines", ctypes.c_uint64), ("total_rows", ctypes.c_uint64),
                ("total_machines", ctypes.c_uint64), ("head", ctypes.c_uint64 * KS_PLC_HEAD_WORDS), ("rows", ctypes.c_void_p), ("machines", ctypes.c_void_p),
                ("pick_type", ctypes.c_void_p), ("pick_zone", ctypes.c_void_p), ("pick_ct", ctypes.c_void_p), ("pick_price", ctypes.c_void_p)]


def _s32(x: int) -> int:
    return x - (1 << 32) if x >= (1 << 31) else x


def decode_placement_head(head) -> dict:
    """A KS_PLC_* head as Python values.  `n_existing`: `where` values below it name existing nodes (for a what-if over a snapshot: node slots), at or above it new nodes."""
    r = [int(x) for x in head]
    return {"id": r[KS_PLC_ID], "pods": r[KS_PLC_P], "n_new": r[KS_PLC_N_NEW], "n_unscheduled": r[KS_PLC_N_UNSCHEDULED], "row_off": r[KS_PLC_ROW_OFF],
            "truncated": bool(r[KS_PLC_FLAGS] & KS_PLC_TRUNCATED), "machines_truncated": bool(r[KS_PLC_FLAGS] & KSH_PROVISION_MACHINES_TRUNCATED), "n_existing": r[KS_PLC_N_EXISTING],
            "reserved": r[7]}


def decode_placement_row(row, n_existing: int) -> dict:
    """A KS_PLC_* row as Python values: `pod`; exactly one of `existing` (a node index / slot) and `new` (new node j) unless the pod is unscheduled (both None); the
    relaxation `stage`; the commit number `seq` (-1 if unscheduled); the packed `reason` word (model.reason_codes unpacks it); the head's id; the queue position."""
    r = [int(x) for x in row]
    where = _s32(r[KS_PLC_POD_WHERE] >> 32)
    return {"pod": r[KS_PLC_POD_WHERE] & 0xFFFFFFFF, "where": where, "existing": where if 0 <= where < n_existing else None, "new": where - n_existing if where >= n_existing else None,
            "stage": _s32(r[KS_PLC_STAGE_SEQ] & 0xFFFFFFFF), "seq": _s32(r[KS_PLC_STAGE_SEQ] >> 32), "reason": r[KS_PLC_REASON_ID] & 0xFFFFFFFF, "id": r[KS_PLC_REASON_ID] >> 32,
            "position": r[KS_PLC_POSITION]}


def placement_lists(rows: Sequence[dict]) -> dict:
    """Decoded rows of ONE problem regrouped as Solve returns them: `new` {j: pods in commit order (Node.Pods)}, `existing` {node: pods in commit order},
    `unscheduled` [pods in queue order], `stage` {pod: stage}, `reasons` {unscheduled pod: packed reason}."""
    new, existing = {}, {}
    for d in sorted((d for d in rows if d["where"] >= 0), key=lambda d: d["seq"]):
        (new.setdefault(d["new"], []) if d["new"] is not None else existing.setdefault(d["existing"], [])).append(d["pod"])
    return {"new": new, "existing": existing, "unscheduled": [d["pod"] for d in rows if d["where"] < 0], "stage": {d["pod"]: d["stage"] for d in rows},
            "reasons": {d["pod"]: d["reason"] for d in rows if d["where"] < 0}}


def placement_rows(flats: Sequence[FlatProblem], ids: Sequence[int], cap_rows: Optional[int] = None, heads=None, rows=None):
    """`ksh_placement_rows`: the placement tables of handles whose results are on the device.  cap_rows None: the sizing call first, then a table exactly large enough.
    `heads` / `rows`: preallocated uint64 tables to fill (tests poison them).  Returns (heads [n, 8], rows [cap_rows, 4] or None, total rows)."""
    import numpy as np
    if len(ids) != len(flats):
        raise ValueError("placement_rows: one id per handle")
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    c_ids = np.ascontiguousarray(np.asarray(list(ids) or [0], dtype=np.uint64))
    kh.ksh_placement_rows.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]

    def call(cap, hd, rw):
        total = ctypes.c_uint64(0)
        rc = kh.ksh_placement_rows(hs, n, c_ids.ctypes.data, hd.ctypes.data, rw.ctypes.data if rw is not None else None, cap, ctypes.byref(total), None)
        if rc != KS_OK:
            raise KSolveError(rc, kh.ksh_last_error().decode())
        return int(total.value)
    if cap_rows is None:
        cap_rows = call(0, np.zeros((max(1, n), KS_PLC_HEAD_WORDS), dtype=np.uint64), None)
    if heads is None:
        heads = np.zeros((max(1, n), KS_PLC_HEAD_WORDS), dtype=np.uint64)
    if rows is None and cap_rows:
        rows = np.zeros((cap_rows, KS_PLC_ROW_WORDS), dtype=np.uint64)
    total = call(cap_rows, heads, rows)
    return heads[:n], rows, total


def provision(snapshot: "ParsedProblem", pod_node: Optional[Sequence[int]], deleting: Sequence[int], words: int, cap_rows: Optional[int] = None, cap_machines: Optional[int] = None,
              device: int = 0, volumes: bool = False, active_resources: bool = False, flags: int = 0, picks: bool = True, rows=None, machines=None):
    """Provisioner.Reconcile's Solve over the snapshot (kshost.h `ksh_provision`): ONE what-if without candidates -- the nodes of `deleting` (the carrier of the pending
    pods first, then the nodes marked for deletion) leave, their pods are the batch.  cap_rows / cap_machines None: the pods bound to `deleting` bound both, read from the
    bindings the library holds or from `pod_node`.  `rows` / `machines`: preallocated uint64 tables to fill (tests poison them).  Returns a dict: `head` (decoded), `rows`
    [total_rows, 4] or None when truncated, `machines` [total_machines, replacement_node_words(words)] or None, `picks` [(type index, zone id, capacity-type id, price) or
    None per machine] or None, `route`, `total_rows`, `total_machines`, `ms`."""
    import numpy as np
    if words < 1:
        raise ValueError("provision: words must be at least 1")
    kh = libs()[1]
    pn, pn_ptr = _pod_node_arg(pod_node)
    dl = _u32s(deleting)
    if cap_rows is None or cap_machines is None:
        bound = list(pod_node) if pod_node is not None else snapshot.bindings()[0]
        gone = set(int(j) for j in deleting)
        npods = sum(1 for b in bound if int(b) in gone)
        cap_rows = npods if cap_rows is None else cap_rows
        cap_machines = npods if cap_machines is None else cap_machines
    if rows is None and cap_rows:
        rows = np.zeros((cap_rows, KS_PLC_ROW_WORDS), dtype=np.uint64)
    if machines is None and cap_machines:
        machines = np.zeros((cap_machines, replacement_node_words(words)), dtype=np.uint64)
    ty, zo, ct = (np.full(max(1, cap_machines), -1, dtype=np.int32) for _ in range(3))
    pr = np.zeros(max(1, cap_machines), dtype=np.float64)
    out = _ProvisionOut()
    out.words, out.cap_rows, out.cap_machines = words, cap_rows, cap_machines
    out.rows = rows.ctypes.data if rows is not None and cap_rows else None
    out.machines = machines.ctypes.data if machines is not None and cap_machines else None
    if picks:
        out.pick_type, out.pick_zone, out.pick_ct, out.pick_price = ty.ctypes.data, zo.ctypes.data, ct.ctypes.data, pr.ctypes.data
    fl = (KSH_DERIVE_VOLUMES if volumes else 0) | (KSH_ACTIVE_RESOURCES if active_resources else 0) | flags
    ms = (ctypes.c_double * 5)()
    kh.ksh_provision.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(_ProvisionOut), ctypes.POINTER(ctypes.c_double)]
    rc = kh.ksh_provision(snapshot._p, fl, pn_ptr, dl.ctypes.data, len(deleting), device, ctypes.byref(out), ms)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    head = decode_placement_head(out.head)
    tr, tm = int(out.total_rows), int(out.total_machines)
    got_machines = tm <= cap_machines and not head["machines_truncated"]
    return {"head": head, "route": PROVISION_ROUTES[int(out.route)], "total_rows": tr, "total_machines": tm, "ms": dict(zip(COMMAND_TIMING_KEYS, [float(x) for x in ms])),
            "rows": None if head["truncated"] else (rows[:tr] if rows is not None else np.zeros((0, KS_PLC_ROW_WORDS), dtype=np.uint64)),
            "machines": (machines[:tm] if machines is not None else np.zeros((0, replacement_node_words(words)), dtype=np.uint64)) if got_machines else None,
            "picks": [None if ty[j] < 0 else (int(ty[j]), int(zo[j]), int(ct[j]), float(pr[j])) for j in range(tm)] if picks and got_machines else None}


def command_rows(flats: Sequence[FlatProblem], ids: Sequence[int], flags: Sequence[int], cand_prices: Sequence[float], type_lists: Sequence[Sequence[Tuple[int, float]]], words: int,
                 out=None, type_off=None):
    """`ksh_command_rows`: the command rows of handles whose results are on the device, the per-what-if inputs given by the caller (flags: KS_CMD_F_*; type_lists[i]:
    (instance-type index, lowest candidate price) per distinct candidate type).  `out`: a preallocated [n, command_row_words(words)] uint64 array to fill (tests poison
    it first); `type_off`: CSR offsets to pass instead of the ones the lists give (tests: malformed offsets).  Returns the rows."""
    import numpy as np
    kh = libs()[1]
    n = len(flats)
    hs = (ctypes.c_void_p * max(1, n))(*[f._h for f in flats])
    c_ids = np.ascontiguousarray(np.asarray(list(ids) or [0], dtype=np.uint64))
    fl, cp = _u32s(flags), np.ascontiguousarray(np.asarray(list(cand_prices) or [0.0], dtype=np.float64))
    off = np.zeros(n + 1, dtype=np.uint32)
    np.cumsum([len(t) for t in type_lists], out=off[1:])
    if type_off is not None:
        off = _u32s(type_off)
    tidx = _u32s(t for ts in type_lists for t, _ in ts)
    tpr = np.ascontiguousarray(np.asarray([p for ts in type_lists for _, p in ts] or [0.0], dtype=np.float64))
    inp = _CommandInputs(fl.ctypes.data, cp.ctypes.data, off.ctypes.data, tidx.ctypes.data, tpr.ctypes.data)
    rows = out if out is not None else np.zeros((max(1, n), command_row_words(words)), dtype=np.uint64)
    kh.ksh_command_rows.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    rc = kh.ksh_command_rows(hs, n, c_ids.ctypes.data, ctypes.byref(inp), words, rows.ctypes.data, None)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return rows[:n]


def decode_command_row(snapshot: "ParsedProblem", row, words: int) -> dict:
    """A command row as Python values, through the handle-free name accessors a C caller has (`ksh_snapshot_name`, `ksh_snapshot_it_state*`): action / reason / narrowed,
    counts, both option stages as instance-type indices, and the replacement's requirements {key: (complement, sorted values, greaterThan, lessThan)}."""
    from .model import LABEL_INSTANCE_TYPE
    kh = libs()[1]
    kh.ksh_snapshot_name.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
    kh.ksh_snapshot_name.restype = ctypes.c_char_p
    kh.ksh_snapshot_it_state.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]
    kh.ksh_snapshot_it_state_value.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32]
    kh.ksh_snapshot_it_state_value.restype = ctypes.c_char_p
    r = [int(x) for x in row]
    dec = r[KS_CMD_DECISION]
    bits = lambda base: [w * 64 + b for w in range(words) for b in range(64) if (r[base + w] >> b) & 1]
    present, complement = r[KS_CMD_PRESENT] & 0xFFFFFFFF, r[KS_CMD_PRESENT] >> 32
    reqs = {}
    for k in range(32):
        if not (present >> k) & 1:
            continue
        key = kh.ksh_snapshot_name(snapshot._p, 0, k, 0).decode()
        vals = tuple(sorted(kh.ksh_snapshot_name(snapshot._p, 1, k, v).decode() for v in range(64) if (r[KS_CMD_MASK + k] >> v) & 1))
        gt, lt = r[KS_CMD_BOUNDS + k] & 0xFFFFFFFF, r[KS_CMD_BOUNDS + k] >> 32
        gt, lt = (gt - (1 << 32) if gt >= (1 << 31) else gt), (lt - (1 << 32) if lt >= (1 << 31) else lt)
        reqs[key] = (bool((complement >> k) & 1), vals, None if gt == -(1 << 31) else gt, None if lt == (1 << 31) - 1 else lt)
    if r[KS_CMD_IT_STATE]:
        c, nv = ctypes.c_int(), ctypes.c_uint32()
        if kh.ksh_snapshot_it_state(snapshot._p, r[KS_CMD_IT_STATE], ctypes.byref(c), ctypes.byref(nv)) != KS_OK:
            raise KSolveError(KS_ERR_INVALID, kh.ksh_last_error().decode())
        reqs[LABEL_INSTANCE_TYPE] = (bool(c.value), tuple(sorted(kh.ksh_snapshot_it_state_value(snapshot._p, r[KS_CMD_IT_STATE], i).decode() for i in range(nv.value))), None, None)
    if (dec >> 16) & 1:      # narrowed to spot (consolidation.go:262-265); "spot" need not be a value of the catalogue's universe
        from .model import LABEL_CAPACITY_TYPE
        reqs[LABEL_CAPACITY_TYPE] = (False, ("spot",), None, None)
    return {"id": r[KS_CMD_ID], "action": dec & 0xFF, "reason": (dec >> 8) & 0xFF, "narrowed": bool((dec >> 16) & 1), "n_new": r[KS_CMD_N_NEW], "n_unscheduled": r[KS_CMD_N_UNSCHEDULED],
            "n_options": r[KS_CMD_N_OPTIONS], "n_options_same_type": r[KS_CMD_N_OPTIONS_SAME_TYPE], "options": bits(KS_CMD_OPTIONS), "options_same_type": bits(KS_CMD_OPTIONS + words),
            "requirements": reqs}


def launch_pick(flats: Sequence[FlatProblem], nodes: Sequence[int]):
    """The launch-time instance-type pick of the reference's in-memory provider (cloudprovider/fake/cloudprovider.go:79-84) on the device, over
    the results the last solve of `flats` left there: for flats[i]'s new node nodes[i], (instance-type index, zone, capacity type, price) of the
    option whose cheapest available offering under the node's zone / capacity-type requirements is cheapest (ties: lowest type index), or None.
    The (zone, capacity type) returned are THAT cheapest offering's.  The in-memory provider labels the launched node with the first
    available offering, in the type's own Offerings order, that is compatible with the requirements (fake/cloudprovider.go:92-102) -- not
    necessarily the cheapest one; the flat problem does not keep the offering order, so callers that need the provider's label choice take
    (type, price) from here and walk the type's Offerings themselves (tests/helpers.py's cluster simulator does)."""
    kh = libs()[1]
    n = len(flats)
    if n == 0:
        return []
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    node = (ctypes.c_uint32 * n)(*[int(x) for x in nodes])
    ty, zo, ct, pr = (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)(), (ctypes.c_double * n)()
    rc = kh.ksh_launch_pick(hs, n, node, ty, zo, ct, pr)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    out = []
    for i in range(n):
        if ty[i] < 0:
            out.append(None)
        else:
            out.append((int(ty[i]), kh.ksh_key_value(flats[i]._h, 0, zo[i]).decode(), kh.ksh_key_value(flats[i]._h, 1, ct[i]).decode(), float(pr[i])))
    return out


def types_subset(flats: Sequence[FlatProblem], nodes: Sequence[int], type_sets: Sequence[Sequence[int]]) -> List[bool]:
    """instanceTypesAreSubset (deprovisioning/helpers.go:118-122) on the device: is type_sets[i] (instance-type indices) a subset of the
    InstanceTypeOptions of flats[i]'s new node nodes[i]?"""
    kh = libs()[1]
    n = len(flats)
    if n == 0:
        return []
    stride = max((f.dims["T"] + 63) // 64 for f in flats)
    hs = (ctypes.c_void_p * n)(*[f._h for f in flats])
    node = (ctypes.c_uint32 * n)(*[int(x) for x in nodes])
    lhs = (ctypes.c_uint64 * (n * stride))()
    for i, ts in enumerate(type_sets):
        for t in ts:
            lhs[i * stride + t // 64] |= 1 << (t % 64)
    out = (ctypes.c_uint32 * n)()
    rc = kh.ksh_types_subset(hs, n, node, lhs, stride, out)
    if rc != KS_OK:
        raise KSolveError(rc, kh.ksh_last_error().decode())
    return [bool(x) for x in out]


def solve_problem(problem: Problem, stats: bool = False, active_resources: bool = False) -> SolveResult:
    fp = FlatProblem(problem, stats=stats, active_resources=active_resources)
    try:
        return fp.solve()
    finally:
        fp.close()


# ---------------------------------------------------------------------------------------------
# Reference-shaped interface
# ---------------------------------------------------------------------------------------------
@dataclass
class SchedulerOptions:
    """scheduling.SchedulerOptions, scheduler.go:36-40."""
    SimulationMode: bool = False
    ActiveResources: bool = False      # not the reference's: flatten over the resource names the batch requests or limits (kshost.h KSH_ACTIVE_RESOURCES); same decisions


@dataclass
class Node:
    """scheduling.Node as its callers read it: embedded MachineTemplate fields + Pods."""
    ProvisionerName: str
    Pods: List[Pod]
    InstanceTypeOptions: List[InstanceType]
    Requirements: Dict[str, object]
    Requests: Dict[str, int]

    def ToMachine(self, provisioner: Optional[Provisioner] = None) -> dict:
        """MachineTemplate.ToMachine (machinetemplate.go:77-100) as far as Solve's result determines it: the requirements
        gain `instance-type In [names of InstanceTypeOptions]` (Requirements.Add = intersection with what is there) and
        are emitted through NodeSelectorRequirements() (requirements.go:80-84, one entry per key); requests are the
        node's accumulated requests.  Labels / taints / kubelet / provider ref come from the provisioner unchanged."""
        from .model import LABEL_INSTANCE_TYPE, RequirementOut
        reqs = dict(self.Requirements)
        names = [it.name for it in self.InstanceTypeOptions]
        cur = reqs.get(LABEL_INSTANCE_TYPE)
        if cur is None:
            merged = RequirementOut(LABEL_INSTANCE_TYPE, False, tuple(names), None, None)
        else:                                   # Intersection of `In names` with the existing requirement (requirement.go:117-150)
            keep = [n for n in names if (n not in cur.values) == cur.complement]
            merged = RequirementOut(LABEL_INSTANCE_TYPE, False, tuple(keep), None, None)
        reqs[LABEL_INSTANCE_TYPE] = merged
        out = {"generateName": self.ProvisionerName,
               "requirements": sorted(r.node_selector_requirement() for r in reqs.values()),
               "resources": {"requests": dict(sorted(self.Requests.items()))}}
        if provisioner is not None:
            out["labels"] = dict(provisioner.labels)
            out["taints"] = [(t.key, t.value, t.effect) for t in provisioner.taints]
        return out


WELL_KNOWN_LABELS = ("karpenter.sh/provisioner-name", "topology.kubernetes.io/zone", "topology.kubernetes.io/region", "node.kubernetes.io/instance-type",
                     "kubernetes.io/arch", "kubernetes.io/os", "karpenter.sh/capacity-type")
RESTRICTED_LABEL_DOMAINS = ("kubernetes.io", "k8s.io", "karpenter.sh")
LABEL_DOMAIN_EXCEPTIONS = ("kops.k8s.io", "node.kubernetes.io", "testing.karpenter.sh")
RESTRICTED_LABELS = ("karpenter.sh/emptiness-timestamp", "kubernetes.io/hostname")


def is_restricted_node_label(key: str, extra_well_known: Sequence[str] = ()) -> bool:
    """v1alpha5.IsRestrictedNodeLabel (labels.go:123-140): labels Karpenter must not put on a node itself."""
    if key in WELL_KNOWN_LABELS or key in extra_well_known:
        return True
    domain = key.split("/", 1)[0] if "/" in key else ""
    if domain in LABEL_DOMAIN_EXCEPTIONS:
        return False
    if any(domain.endswith(d) for d in RESTRICTED_LABEL_DOMAINS):
        return True
    return key in RESTRICTED_LABELS


def requirements_labels(requirements: Dict[str, object], extra_well_known: Sequence[str] = ()) -> Dict[str, str]:
    """Requirements.Labels() (requirements.go:208-218) -- the labels MachineTemplate.ToNode puts on the node object besides the provisioner's own
    (machinetemplate.go:62-74): for every key that is not restricted, Requirement.Any() (requirement.go:152-168).  Any() draws at random where the
    reference leaves a choice (one of the In values; an integer in (gt, lt) for NotIn / Exists); this mirror takes the smallest admissible one."""
    out: Dict[str, str] = {}
    for key, r in requirements.items():
        if is_restricted_node_label(key, extra_well_known):
            continue
        if not r.complement:
            if r.values:                                        # In
                out[key] = sorted(r.values)[0]
            continue                                            # DoesNotExist: ""
        lo_ = 0 if r.greater_than is None else r.greater_than + 1      # NotIn / Exists
        out[key] = str(lo_)
    return out


@dataclass
class ExistingNode:
    """scheduling.ExistingNode: the state node plus the pods Solve placed on it."""
    Node: StateNode
    Pods: List[Pod]


class Scheduler:
    """scheduling.Scheduler (scheduler.go:81-94)."""

    def __init__(self, provisioners, instance_types, state_nodes, daemonset_pods, cluster_pods, extra_well_known, opts):
        self.provisioners, self.instance_types, self.state_nodes = provisioners, instance_types, state_nodes
        self.daemonset_pods, self.cluster_pods, self.extra_well_known, self.opts = daemonset_pods, cluster_pods, extra_well_known, opts

    def Solve(self, pods: Sequence[Pod]) -> Tuple[List[Node], List[ExistingNode], None]:
        problem = Problem(instance_types=self.instance_types, provisioners=self.provisioners, pods=list(pods),
                          daemonset_pods=self.daemonset_pods, nodes=self.state_nodes, cluster_pods=self.cluster_pods,
                          extra_well_known=self.extra_well_known, simulation_mode=self.opts.SimulationMode)
        res = solve_problem(problem, active_resources=self.opts.ActiveResources)
        self.last_result = res
        by_name = {it.name: it for it in self.instance_types}
        nodes = [Node(n.provisioner, [pods[i] for i in n.pods], [by_name[x] for x in n.instance_types], n.requirements, n.requests)
                 for n in res.new_nodes]
        state = {n.name: n for n in self.state_nodes}
        existing = [ExistingNode(state[name], [pods[i] for i in idxs]) for name, idxs in res.existing.items()]
        return nodes, existing, None


def NewScheduler(provisioners: Sequence[Provisioner], instance_types: Sequence[InstanceType],
                 state_nodes: Sequence[StateNode] = (), daemonset_pods: Sequence[Pod] = (),
                 cluster_pods: Sequence[ClusterPod] = (), extra_well_known: Sequence[str] = (),
                 opts: Optional[SchedulerOptions] = None) -> Scheduler:
    """provisioning.(*Provisioner).NewScheduler (provisioner.go:237-296): every provisioner offers the
    instance types listed in `Provisioner.instance_types` (indices into `instance_types`)."""
    return Scheduler(list(provisioners), list(instance_types), list(state_nodes), list(daemonset_pods), list(cluster_pods),
                     list(extra_well_known), opts or SchedulerOptions())
