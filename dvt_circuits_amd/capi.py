"""ctypes binding of include/dvt_prover.h.  Loads the in-tree HIP library
`dvt_circuits_amd/libdvt_prover.so`; raises if it is missing — there is no
fallback path."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdvt_prover.so")
CSRC = os.path.join(HERE, "csrc")

DVT_OK, DVT_ERR_GUEST, DVT_ERR_INPUT, DVT_ERR_DEVICE, DVT_ERR_UNSUPPORTED, DVT_ERR_REJECTED = 0, 1, 2, 3, 4, 5
PATHS = {"default": 0, "rows": 1, "parts": 2}             # DVT_PATH_* (K4 / K5 launches)
SELECTORS = {"table": 0, "kernel": 1}                     # DVT_SELECTORS_*
DVT_KEEP_NONE, DVT_KEEP_TREE, DVT_KEEP_FULL = 0, 1, 2     # what a committed shard keeps in HBM for phase 2 ("keep_phase1")
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)


class DevMatrix(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("width", C.c_uint32), ("log_height", C.c_uint32)]


class HostTrace(C.Structure):
    _fields_ = [("chip_id", C.c_uint32), ("log_n", C.c_uint32), ("data", u32p)]


class PathChain(C.Structure):
    _fields_ = [("start", C.POINTER(C.c_uint32)), ("depth", C.c_uint32), ("leaf", C.c_uint32), ("siblings", C.POINTER(C.c_uint32)),
                ("inject", C.POINTER(C.c_uint32)), ("inject_at", C.POINTER(C.c_uint8)), ("root", C.POINTER(C.c_uint32))]


class DvtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dvt error {code}: {msg}")
        self.code = code
        self.msg = msg


def build():
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc); there is no CPU fallback")
    try:
        # PyTorch bundles its own HIP runtime; whichever runtime initialises the GPU first owns it, so
        # when torch is going to be used in this process (device-memory plumbing) it must be loaded first.
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    lib.dvt_abi_version.restype = u32
    lib.dvt_prover_create.argtypes = [C.c_char_p, C.POINTER(vp)]
    lib.dvt_prover_destroy.argtypes = [vp]
    lib.dvt_prover_destroy.restype = None
    lib.dvt_last_error.argtypes = [vp]
    lib.dvt_last_error.restype = C.c_char_p
    lib.dvt_free.argtypes = [vp]
    lib.dvt_free.restype = None
    lib.dvt_stream.argtypes = [vp]
    lib.dvt_stream.restype = vp
    lib.dvt_sync.argtypes = [vp]
    lib.dvt_prover_device_count.argtypes = [vp]
    lib.dvt_prover_device_count.restype = u32
    lib.dvt_prover_device.argtypes = [vp, u32]
    lib.dvt_prover_device.restype = C.c_int
    lib.dvt_dev_to_internal.argtypes = [vp, vp, sz]
    lib.dvt_dev_from_internal.argtypes = [vp, vp, sz]
    lib.dvt_stage_coset_lde.argtypes = [vp, vp, vp, vp, u32, u32, u32]
    lib.dvt_merkle_digest_words.argtypes = [C.POINTER(DevMatrix), sz]
    lib.dvt_merkle_digest_words.restype = sz
    lib.dvt_stage_merkle_commit.argtypes = [vp, C.POINTER(DevMatrix), sz, vp]
    lib.dvt_stage_poseidon2_permute.argtypes = [vp, vp, sz]
    lib.dvt_stage_fri_fold.argtypes = [vp, vp, vp, vp, u32p, u32]
    lib.dvt_stage_logup_running_sum.argtypes = [vp, vp, vp, u32, u32p]
    lib.dvt_stage_open.argtypes = [vp, C.POINTER(DevMatrix), sz, u32p, u32p]
    lib.dvt_stage_reduced_opening.argtypes = [vp, C.POINTER(vp), u32, u32, u32, u32p, u32p, u32p, u32p, vp]
    lib.dvt_stage_pow_grind.argtypes = [vp, u32p, u32, u32, u32p]
    lib.dvt_stage_perm.argtypes = [vp, C.c_char_p, u32, vp, vp, u32, u32p, u32p, u32p, u32, vp, u32p]
    lib.dvt_stage_quotient.argtypes = [vp, C.c_char_p, u32, vp, vp, vp, u32, u32p, u32p, u32p, u32p, u32p, u32, u32, vp]
    lib.dvt_stage_check_constraints.argtypes = [vp, C.c_char_p, u32, vp, vp, u32, u32p, u32p, u32p, C.POINTER(CheckResult)]
    lib.dvt_stage_bus_sums.argtypes = [vp, C.c_char_p, u32, vp, vp, u32, u32p, u32p, u32p, u32p]
    lib.dvt_rv32_check_job.argtypes = [vp, vp, vp, C.POINTER(CheckFinding), sz, C.POINTER(CheckSummary)]
    lib.dvt_stage_bus_ledger_new.argtypes = [vp, C.c_char_p, u32, u32, C.c_uint64, C.POINTER(vp)]
    lib.dvt_stage_bus_ledger_add.argtypes = [vp, vp, u32, vp, vp, u32, u32p, u32]
    lib.dvt_stage_bus_ledger_collect.argtypes = [vp, vp, u32, vp, vp, u32, u32p, u32]
    lib.dvt_stage_bus_ledger_add_tuple.argtypes = [vp, vp, u32, u32p, u32, C.c_int32, u32, u32]
    lib.dvt_stage_bus_ledger_close.argtypes = [vp, vp, u32p]
    lib.dvt_stage_bus_ledger_result.argtypes = [vp, vp, C.POINTER(BusTuple), sz, C.POINTER(sz), u32p]
    lib.dvt_stage_bus_ledger_free.argtypes = [vp, vp]
    lib.dvt_rv32_job_bus_tuples.argtypes = [vp, vp, vp, C.POINTER(BusTuple), sz, C.POINTER(sz), u32p]
    lib.dvt_debug_ledger_key.argtypes = [C.c_uint64, u32, u32, u32p]
    u64 = C.c_uint64
    lib.dvt_stage_hunt_cells.argtypes = [vp, C.c_char_p, u32, vp, vp, u32, u32p, u64, u32p, u32, u32, u32, u64, u32p, u8p]
    lib.dvt_stage_hunt_pairs.argtypes = [vp, C.c_char_p, u32, vp, vp, u32, u32p, u64, u32p, u32, u32p, u32, u32, u32, u32, u64,
                                         C.POINTER(Escape), sz, C.POINTER(u64), C.POINTER(u64)]
    lib.dvt_rv32_hunt_shard.argtypes = [vp, vp, vp, sz, u32, u64, u32p, u32, u32, u32p, u32, u32, u32, u32, u64, u32p, u8p,
                                        C.POINTER(Escape), sz, C.POINTER(u64), C.POINTER(u64)]
    lib.dvt_debug_ledger_key.restype = C.c_uint64
    lib.dvt_stage_hunt_join_new.argtypes = [vp, C.c_char_p, u64, u32p, u32, sz, sz, u32, C.POINTER(vp)]
    lib.dvt_stage_hunt_join_supply.argtypes = [vp, vp, u32, vp, vp, u32, u32p]
    lib.dvt_stage_hunt_join_add.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32p, u32, u32, u32p, u32, u64]
    lib.dvt_stage_hunt_join_match.argtypes = [vp, vp, C.POINTER(JoinSummary)]
    lib.dvt_stage_hunt_join_result.argtypes = [vp, vp, C.POINTER(JoinCell), sz, C.POINTER(sz), C.POINTER(JoinCell), sz, C.POINTER(sz)]
    lib.dvt_stage_hunt_join_free.argtypes = [vp, vp]
    lib.dvt_rv32_hunt_join_job.argtypes = [vp, vp, vp, C.POINTER(JoinWindow), sz, u32p, u32, u64, u32p, u32, u32p, u32p, u64, sz, sz, u32,
                                           C.POINTER(JoinSummary), C.POINTER(JoinCell), sz, C.POINTER(sz), C.POINTER(JoinCell), sz, C.POINTER(sz)]
    lib.dvt_rv32_job_shard_chips.argtypes = [vp, sz]
    lib.dvt_rv32_job_shard_chips.restype = u32
    lib.dvt_rv32_job_shard_chip_shape.argtypes = [vp, sz, u32, u32p, u32p]
    lib.dvt_machine_setup.argtypes = [vp, C.c_char_p, C.POINTER(HostTrace), sz, C.POINTER(vp), C.POINTER(u8p), C.POINTER(sz)]
    lib.dvt_pk_free.argtypes = [vp, vp]
    lib.dvt_pk_free.restype = None
    lib.dvt_machine_prove.argtypes = [vp, vp, C.POINTER(HostTrace), sz, u32p, sz, C.POINTER(u8p), C.POINTER(sz)]
    lib.dvt_machine_verify.argtypes = [C.c_char_p, sz, C.c_char_p, sz, u32, u32, C.POINTER(C.c_char_p)]
    lib.dvt_prover_machine_verify.argtypes = [vp, C.c_char_p, sz, C.c_char_p, sz, u32, u32, C.POINTER(C.c_char_p)]
    lib.dvt_prover_verify.argtypes = [vp, C.c_char_p, sz, C.c_char_p, sz, u32, u32, C.POINTER(C.c_int32), C.POINTER(u8p), C.POINTER(sz), C.POINTER(C.c_char_p)]
    lib.dvt_prover_verify_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_stage_sponge_rows.argtypes = [vp, u32p, u32p, sz, u32p]
    lib.dvt_stage_verify_paths.argtypes = [vp, C.POINTER(PathChain), sz, u8p]
    lib.dvt_stage_multipath_nodes.argtypes = [u32, u32p, sz, u32p, sz, C.POINTER(sz)]
    lib.dvt_stage_verify_multipath.argtypes = [vp, u32, u32p, u32p, sz, u8p, u32p, u32p, sz, u32p, u8p]
    for fn in (lib.dvt_proof_compact, lib.dvt_proof_expand):
        fn.argtypes = [C.c_char_p, sz, C.c_char_p, sz, u32, u32, C.POINTER(u8p), C.POINTER(sz), C.POINTER(C.c_char_p)]
    lib.dvt_debug_compact_list_sweep.argtypes = [C.c_char_p, sz, C.c_char_p, sz, u32, u32, C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_char_p)]
    lib.dvt_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.dvt_setup.argtypes = [vp, C.c_char_p, sz, C.POINTER(vp), C.POINTER(u8p), C.POINTER(sz)]
    lib.dvt_execute.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, C.c_uint64, C.POINTER(u8p), C.POINTER(sz), C.POINTER(Report), C.POINTER(C.c_char_p)]
    lib.dvt_execute_io.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, C.c_uint64, C.POINTER(u8p), C.POINTER(sz), C.POINTER(u8p), C.POINTER(sz), C.POINTER(Report), C.POINTER(C.c_char_p)]
    lib.dvt_debug_exec_rate.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u32, C.c_int]
    lib.dvt_debug_exec_rate.restype = C.c_double
    lib.dvt_debug_p2_f64_selfcheck.argtypes = [u32, u32]
    lib.dvt_debug_p2_f64_selfcheck.restype = u64
    lib.dvt_debug_p2_f64_sbox_check.argtypes = [u32, u32, C.POINTER(C.c_double)]
    lib.dvt_debug_p2_f64_sbox_check.restype = u64
    lib.dvt_debug_ntt_group_check.argtypes = [u32, u32] + [C.POINTER(C.c_double)] * 3
    lib.dvt_debug_ntt_group_check.restype = u64
    lib.dvt_prove_core.argtypes = [vp, vp, C.POINTER(Buf), sz, C.POINTER(u8p), C.POINTER(sz), C.POINTER(Report)]
    lib.dvt_verify.argtypes = [C.c_char_p, sz, C.c_char_p, sz, u32, u32, C.POINTER(C.c_int32), C.POINTER(u8p), C.POINTER(sz), C.POINTER(C.c_char_p)]
    lib.dvt_rv32_prepare.argtypes = [vp, vp, C.POINTER(Buf), sz, C.POINTER(vp), C.POINTER(Report)]
    lib.dvt_rv32_prepare_part.argtypes = [vp, vp, C.POINTER(Buf), sz, sz, sz, C.POINTER(vp), C.POINTER(Report)]
    lib.dvt_rv32_header_words.restype = u32
    lib.dvt_rv32_job_exec_wait_seconds.argtypes = [vp]
    lib.dvt_rv32_job_exec_wait_seconds.restype = C.c_double
    lib.dvt_rv32_prove_job.argtypes = [vp, vp, vp, C.POINTER(u8p), C.POINTER(sz)]
    lib.dvt_job_free.argtypes = [vp, vp]
    lib.dvt_job_free.restype = None
    lib.dvt_rv32_debug_traces.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u32, u32, u32p, C.POINTER(u32p), C.POINTER(sz), C.POINTER(C.c_char_p)]
    lib.dvt_rv32_job_shards.argtypes = [vp]
    lib.dvt_rv32_job_shards.restype = sz
    lib.dvt_rv32_job_shard_member.argtypes = [vp, sz]
    lib.dvt_rv32_job_shard_member.restype = C.c_int
    lib.dvt_rv32_job_shard_device_rows.argtypes = [vp, sz]
    lib.dvt_rv32_job_shard_device_rows.restype = u32
    lib.dvt_rv32_job_shard_kept.argtypes = [vp, sz]
    lib.dvt_rv32_job_shard_kept.restype = C.c_int
    lib.dvt_rv32_job_shard_kept_bytes.argtypes = [vp, sz]
    lib.dvt_rv32_job_shard_kept_bytes.restype = C.c_uint64
    lib.dvt_debug_keep_plan.argtypes = [C.c_int, u64, u64, u64, u64, u64, u64, u64, C.c_int, C.c_int64, u64]
    lib.dvt_debug_keep_plan.restype = C.c_int
    lib.dvt_rv32_commit_shard.argtypes = [vp, vp, vp, sz, u32p]
    lib.dvt_rv32_challenges.argtypes = [C.c_char_p, sz, u32p, sz, u32p]
    lib.dvt_rv32_prove_shard.argtypes = [vp, vp, vp, sz, u32p, C.POINTER(u8p), C.POINTER(sz)]
    lib.dvt_rv32_assemble.argtypes = [vp, C.POINTER(C.c_char_p), C.POINTER(sz), sz, C.POINTER(u8p), C.POINTER(sz)]
    lib.dvt_rv32_debug_device_traces.argtypes = [vp, vp, vp, sz, C.POINTER(u32p), C.POINTER(sz)]
    lib.dvt_rv32_debug_poke_cell.argtypes = [vp, vp, sz, u32, u32, u32, u32]
    prof_out = [C.POINTER(u64), sz, C.POINTER(ProfileEdge), sz, C.POINTER(ProfileSyscall), sz, C.POINTER(ProfileOpcode), sz, C.POINTER(ProfileSummary)]
    lib.dvt_rv32_job_profile.argtypes = [vp, vp, vp, u32] + prof_out
    lib.dvt_execute_profile.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64] + prof_out + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    tree_out = [C.POINTER(CalltreeArc), sz, C.POINTER(CalltreeFunc), sz, C.POINTER(CalltreeSummary)]
    lib.dvt_rv32_job_calltree.argtypes = [vp, vp, vp, u32] + tree_out
    lib.dvt_rv32_job_calltree_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_execute_calltree.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64] + tree_out + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    mem_out = [C.POINTER(u64), sz, C.POINTER(MemoryPage), sz, C.POINTER(MemorySummary)]
    lib.dvt_rv32_job_memory.argtypes = [vp, vp, vp] + mem_out
    lib.dvt_execute_memory.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64] + mem_out + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    watch_io = [C.POINTER(WatchQuery), sz, sz, C.POINTER(WatchHit), C.POINTER(u64), C.POINTER(WatchSummary)]
    lib.dvt_rv32_job_watch.argtypes = [vp, vp, vp] + watch_io
    lib.dvt_rv32_job_watch_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_execute_watch.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64, u32] + watch_io + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    snap_io = [u32, u32, C.POINTER(SnapRange), sz, C.POINTER(SnapCell), C.POINTER(SnapCell), sz, C.POINTER(SnapFrame), sz, C.POINTER(SnapSummary)]
    lib.dvt_rv32_job_snapshot.argtypes = [vp, vp, vp] + snap_io
    lib.dvt_rv32_job_snapshot_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_execute_snapshot.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64, u32] + snap_io + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    origin_io = [u32, u32, u32, u32, u32, u32, C.POINTER(OriginNode), sz, C.POINTER(OriginEdge), sz, C.POINTER(OriginSummary)]
    lib.dvt_rv32_job_origin.argtypes = [vp, vp, vp] + origin_io
    lib.dvt_rv32_job_origin_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_execute_origin.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64, u32] + origin_io + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    uses_io = [u32, u32, u32, u32, u32, u32, u32, C.POINTER(UsesNode), sz, C.POINTER(UsesDef), sz, C.POINTER(UsesEdge), sz, C.POINTER(UsesSummary)]
    lib.dvt_rv32_job_uses.argtypes = [vp, vp, vp] + uses_io
    lib.dvt_rv32_job_uses_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_execute_uses.argtypes = [C.c_char_p, sz, C.POINTER(Buf), sz, u64, u32] + uses_io + [C.POINTER(Report), C.POINTER(C.c_char_p)]
    diverge_io = [DivergePos, DivergePos, u64, u32, u32, sz, C.POINTER(DivergePair), C.POINTER(DivergePair), C.POINTER(DivergeReg), C.POINTER(DivergeSummary)]
    lib.dvt_rv32_job_diverge.argtypes = [vp, vp, vp, vp] + diverge_io
    lib.dvt_rv32_job_diverge_times.argtypes = [vp, C.POINTER(C.c_double)]
    lib.dvt_execute_diverge.argtypes = [C.c_char_p, sz, C.c_char_p, sz, C.c_char_p, sz, u64, u32] + diverge_io + \
                                       [C.POINTER(Report), C.POINTER(Report), C.POINTER(C.c_char_p)]
    lib.dvt_stdin_from_json.argtypes = [C.c_char_p, C.c_char_p, sz, C.c_int, C.POINTER(u8p), C.POINTER(sz), C.POINTER(C.c_char_p)]
    _lib = lib
    return lib


class CheckResult(C.Structure):
    _fields_ = [("violations", C.c_uint64), ("first_row", C.c_uint32), ("first_constraint", C.c_int32)]


class CheckFinding(C.Structure):
    _fields_ = [("shard", C.c_uint32), ("chip", C.c_uint32), ("log_n", C.c_uint32), ("r", CheckResult)]


class CheckSummary(C.Structure):
    _fields_ = [("violations", C.c_uint64), ("n_findings", C.c_uint32), ("bus_checked", C.c_uint32), ("unbalanced_buses", C.c_uint32),
                ("ms", C.c_float)]


CHECK_BUSES = 8   # DVT_CHECK_BUSES
LEDGER_MAX_ARITY = 40   # DVT_LEDGER_MAX_ARITY
HOST_CHIP = 0xffffffff  # first_chip of a tuple whose lowest occurrence the caller added


class BusTuple(C.Structure):
    """dvt_bus_tuple: a tuple of a LogUp bus whose signed multiplicities do not cancel"""
    _fields_ = [("bus", C.c_uint32), ("arity", C.c_uint32), ("net", C.c_uint32), ("n_send", C.c_uint32), ("n_recv", C.c_uint32),
                ("first_tag", C.c_uint32), ("first_chip", C.c_uint32), ("first_row", C.c_uint32), ("first_interaction", C.c_uint32),
                ("values", C.c_uint32 * LEDGER_MAX_ARITY)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_[:9]}
        d["values"] = [int(x) for x in self.values[:min(self.arity, LEDGER_MAX_ARITY)]]
        return d


def _bus_tuples(arr, n):
    """the first n records of a BusTuple array as dicts (through numpy: a ledger may return hundreds of thousands)"""
    if not n:
        return []
    names = [k for k, _ in BusTuple._fields_[:9]]
    rows = np.frombuffer(arr, np.uint32).reshape(-1, 9 + LEDGER_MAX_ARITY)[:n].tolist()
    return [dict(zip(names, r[:9]), values=r[9:9 + min(r[1], LEDGER_MAX_ARITY)]) for r in rows]


HUNT_MAX_DELTAS = 8   # DVT_HUNT_MAX_DELTAS


class Escape(C.Structure):
    """dvt_escape: a pair of changes that nothing rejects although one of them alone is rejected"""
    _fields_ = [("row", C.c_uint32), ("n_cells", C.c_uint32), ("col", C.c_uint32 * 2), ("row_off", C.c_uint32 * 2),
                ("delta", C.c_uint32 * 2), ("alone", C.c_uint32)]


def _escapes(arr, n):
    """the first n records of an Escape array as dicts"""
    if not n:
        return []
    rows = np.frombuffer(arr, np.uint32).reshape(-1, 9)[:n].tolist()
    return [dict(row=r[0], n_cells=r[1], col=r[2:4], row_off=r[4:6], delta=r[6:8], alone=r[8]) for r in rows]


JOIN_TRUNC_RECORDS, JOIN_TRUNC_ABSORBED, JOIN_TRUNC_PROBES, JOIN_TRUNC_OUTPUT = 1, 2, 4, 8   # DVT_JOIN_TRUNC_*
JOIN_NO_GROUP = 0xffffffff


class JoinCell(C.Structure):
    """dvt_join_cell: one changed cell of a group of the join hunt, or an absorbed cell (group JOIN_NO_GROUP)"""
    _fields_ = [("group", C.c_uint32), ("side", C.c_uint32), ("tag", C.c_uint32), ("chip", C.c_uint32), ("col", C.c_uint32),
                ("row", C.c_uint32), ("delta", C.c_uint32)]


class JoinSummary(C.Structure):
    """dvt_join_summary"""
    _fields_ = [("candidates", C.c_uint64), ("open_emitted", C.c_uint64), ("open_stored", C.c_uint64), ("absorbed_emitted", C.c_uint64),
                ("absorbed_stored", C.c_uint64), ("matched", C.c_uint64), ("groups", C.c_uint64), ("pairs", C.c_uint64),
                ("truncated", C.c_uint32), ("reserved", C.c_uint32)]


class JoinWindow(C.Structure):
    """dvt_join_window: rows of one chip table of one shard of a job (row_count 0: to the end of the table)"""
    _fields_ = [("shard", C.c_uint32), ("chip", C.c_uint32), ("row_first", C.c_uint32), ("row_count", C.c_uint32)]


def _join_result(sm, cells, n_cells, cap_cells, soaked, n_soaked, cap_soaked):
    """what Prover.hunt_join and Prover.hunt_join_job return"""
    summary = {k: int(getattr(sm, k)) for k, _ in JoinSummary._fields_ if k != "reserved"}
    if n_cells > cap_cells:
        summary["truncated"] |= JOIN_TRUNC_OUTPUT
    groups = []
    for c in _join_cells(cells, min(n_cells, cap_cells)):
        while len(groups) <= c["group"]:
            groups.append([[], []])
        groups[c["group"]][c["side"]].append({k: c[k] for k in ("tag", "chip", "col", "row", "delta")})
    absorbed = [{k: c[k] for k in ("tag", "chip", "col", "row", "delta")} for c in _join_cells(soaked, min(n_soaked, cap_soaked))]
    return dict(summary=summary, groups=groups, absorbed=absorbed)


def _join_cells(arr, n):
    """the first n records of a JoinCell array as dicts"""
    if not n:
        return []
    names = [k for k, _ in JoinCell._fields_]
    return [dict(zip(names, r)) for r in np.frombuffer(arr, np.uint32).reshape(-1, 7)[:n].tolist()]


class BusLedger:
    """The stage-level bus ledger (dvt_stage_bus_ledger_*): add / add_tuple every table and tuple, close(), and when it
    reports dirty buckets collect / add_tuple the same again, then result().  Matrices as Prover.stage_bus_sums takes them."""

    def __init__(self, prover, machine, log_buckets=20, cap_slots=1 << 16, seed=1):
        self.p, self.machine = prover, machine
        h = C.c_void_p()
        prover.check(prover.lib.dvt_stage_bus_ledger_new(prover.h, machine.encode(), log_buckets, cap_slots, seed, C.byref(h)))
        self.h = h

    def _rows(self, fn, chip, t_main, t_prep, log_n, pubs, tag):
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.p.check(fn(self.p.h, self.h, chip, ptr(t_main), ptr(t_prep), log_n, pv, tag))

    def add(self, chip, t_main, t_prep, log_n, pubs, tag=0):
        self._rows(self.p.lib.dvt_stage_bus_ledger_add, chip, t_main, t_prep, log_n, pubs, tag)

    def collect(self, chip, t_main, t_prep, log_n, pubs, tag=0):
        self._rows(self.p.lib.dvt_stage_bus_ledger_collect, chip, t_main, t_prep, log_n, pubs, tag)

    def add_tuple(self, bus, values, sign, mult, tag=0):
        v = (C.c_uint32 * max(len(values), 1))(*[int(x) for x in values])
        self.p.check(self.p.lib.dvt_stage_bus_ledger_add_tuple(self.p.h, self.h, bus, v, len(values), sign, mult, tag))

    def close(self):
        n = C.c_uint32()
        self.p.check(self.p.lib.dvt_stage_bus_ledger_close(self.p.h, self.h, C.byref(n)))
        return int(n.value)

    def result(self, cap=1 << 16):
        """(tuples as dicts sorted by (bus, values), truncated)"""
        arr = (BusTuple * max(cap, 1))()
        n, trunc = C.c_size_t(), C.c_uint32()
        self.p.check(self.p.lib.dvt_stage_bus_ledger_result(self.p.h, self.h, arr, cap, C.byref(n), C.byref(trunc)))
        return _bus_tuples(arr, n.value), bool(trunc.value)

    def free(self):
        if self.h:
            self.p.check(self.p.lib.dvt_stage_bus_ledger_free(self.p.h, self.h))
            self.h = None


class Buf(C.Structure):
    _fields_ = [("data", C.c_char_p), ("len", C.c_size_t)]


class Report(C.Structure):
    _fields_ = [("cycles", C.c_uint64), ("exit_code", C.c_int32), ("halted", C.c_uint32), ("unprovable", C.c_uint32)]


def _bufs(stdin):
    arr = (Buf * max(len(stdin), 1))()
    for i, b in enumerate(stdin):
        arr[i] = Buf(bytes(b), len(b))
    return arr


def _take_str(lib, p):
    s = p.value.decode() if p.value else ""
    if p.value:
        lib.dvt_free(C.cast(p, C.c_void_p))
    return s


def execute(elf: bytes, stdin=(), max_cycles=0):
    """Host-only emulation (reference src/main.rs:430-447).  Returns (rc, report dict, public_values, error text)."""
    lib = load()
    pv, n, rep, err = u8p(), C.c_size_t(), Report(), C.c_char_p()
    rc = lib.dvt_execute(elf, len(elf), _bufs(stdin), len(stdin), max_cycles, C.byref(pv), C.byref(n), C.byref(rep), C.byref(err))
    out = C.string_at(pv, n.value) if pv else b""
    if pv:
        lib.dvt_free(C.cast(pv, C.c_void_p))
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), out, _take_str(lib, err)


class ProfileEdge(C.Structure):
    _fields_ = [("from_pc", C.c_uint32), ("to_pc", C.c_uint32), ("count", C.c_uint64)]


class ProfileSyscall(C.Structure):
    _fields_ = [("id", C.c_uint32), ("pad", C.c_uint32), ("count", C.c_uint64)]


class ProfileOpcode(C.Structure):
    _fields_ = [("name", C.c_char * 8), ("count", C.c_uint64)]


class ProfileSummary(C.Structure):
    _fields_ = [("cycles", C.c_uint64), ("n_transfers", C.c_uint64), ("dropped_transfers", C.c_uint64), ("text_base", C.c_uint32),
                ("n_instr", C.c_uint32), ("n_edges", C.c_uint32), ("n_syscalls", C.c_uint32), ("n_opcodes", C.c_uint32),
                ("shards_tallied", C.c_uint32), ("shards_total", C.c_uint32), ("ms", C.c_float)]


def _profile(call):
    """The execution report through call(pc_count, cap_pc, edges, cap_edges, sys, cap_sys, ops, cap_ops, summary) -> rc: once
    for the sizes, once for the tables.  Returns (rc, report), report = None when the first call fails without a summary,
    else dict(summary, pc_count (numpy u64), edges = [(from_pc, to_pc, count)], syscalls = {id: count}, opcodes = {name: count})."""
    s = ProfileSummary()
    rc = call(None, 0, None, 0, None, 0, None, 0, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    pc = np.zeros(max(int(s.n_instr), 1), np.uint64)
    edges, sys_, ops = (ProfileEdge * max(int(s.n_edges), 1))(), (ProfileSyscall * max(int(s.n_syscalls), 1))(), (ProfileOpcode * max(int(s.n_opcodes), 1))()
    rc = call(pc.ctypes.data_as(C.POINTER(C.c_uint64)), int(s.n_instr), edges, int(s.n_edges), sys_, int(s.n_syscalls), ops, int(s.n_opcodes), C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    summary = {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in ProfileSummary._fields_}
    return rc, dict(summary=summary, pc_count=pc[:int(s.n_instr)],
                    edges=[(int(e.from_pc), int(e.to_pc), int(e.count)) for e in edges[:int(s.n_edges)]],
                    syscalls={int(e.id): int(e.count) for e in sys_[:int(s.n_syscalls)]},
                    opcodes={e.name.decode(): int(e.count) for e in ops[:int(s.n_opcodes)]})


def execute_profile(elf: bytes, stdin=(), max_cycles=0):
    """Host-only execution report (dvt_execute_profile): the guest in trace mode, tallied shard by shard.  Returns (rc, report
    dict as execute() gives it, profile dict as Prover.job_profile gives it or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)

    def call(*out):
        if err.value:
            lib.dvt_free(C.cast(err, C.c_void_p))
        return lib.dvt_execute_profile(elf, len(elf), bufs, len(stdin), max_cycles, *out, C.byref(rep), C.byref(err))
    rc, prof = _profile(call)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), prof, _take_str(lib, err)


class CalltreeArc(C.Structure):
    _fields_ = [("caller_pc", C.c_uint32), ("callee_pc", C.c_uint32), ("calls", C.c_uint64), ("cycles", C.c_uint64)]


class CalltreeFunc(C.Structure):
    _fields_ = [("pc", C.c_uint32), ("pad", C.c_uint32), ("calls", C.c_uint64), ("inclusive", C.c_uint64), ("self", C.c_uint64)]


class CalltreeSummary(C.Structure):
    _fields_ = [("cycles", C.c_uint64), ("n_frames", C.c_uint64), ("dropped_frames", C.c_uint64), ("dropped_cycles", C.c_uint64),
                ("unmatched_returns", C.c_uint64), ("text_base", C.c_uint32), ("n_instr", C.c_uint32), ("n_arcs", C.c_uint32),
                ("n_funcs", C.c_uint32), ("max_depth", C.c_uint32), ("open_at_exit", C.c_uint32), ("shards_total", C.c_uint32), ("ms", C.c_float)]


NO_FN = 0xffffffff   # caller_pc of the root's arc


def _calltree(call):
    """The call-tree report through call(arcs, cap_arcs, funcs, cap_funcs, summary) -> rc: once for the sizes, once for the
    tables.  Returns (rc, report), report = None when a call fails without a summary, else dict(summary, arcs = [(caller_pc or
    None for the root, callee_pc, calls, cycles)], funcs = [(pc, calls, inclusive, self)])."""
    s = CalltreeSummary()
    rc = call(None, 0, None, 0, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    n_arcs, n_funcs = int(s.n_arcs), int(s.n_funcs)
    arcs, funcs = (CalltreeArc * max(n_arcs, 1))(), (CalltreeFunc * max(n_funcs, 1))()
    rc = call(arcs, n_arcs, funcs, n_funcs, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    summary = {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in CalltreeSummary._fields_}
    a = np.frombuffer(arcs, np.dtype([("caller", "<u4"), ("callee", "<u4"), ("calls", "<u8"), ("cycles", "<u8")]))[:min(n_arcs, int(s.n_arcs))].tolist()
    f = np.frombuffer(funcs, np.dtype([("pc", "<u4"), ("pad", "<u4"), ("calls", "<u8"), ("inclusive", "<u8"), ("self", "<u8")]))[:min(n_funcs, int(s.n_funcs))].tolist()
    return rc, dict(summary=summary, arcs=[(None if c == NO_FN else c, d, n, cyc) for c, d, n, cyc in a],
                    funcs=[(pc, n, inc, own) for pc, _, n, inc, own in f])


def execute_calltree(elf: bytes, stdin=(), max_cycles=0):
    """Host-only call-tree report (dvt_execute_calltree): inclusive and self cycles per function and per caller -> callee arc.
    Returns (rc, report dict as execute() gives it, call-tree dict as Prover.job_calltree gives it or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)

    def call(*out):
        if err.value:
            lib.dvt_free(C.cast(err, C.c_void_p))
        return lib.dvt_execute_calltree(elf, len(elf), bufs, len(stdin), max_cycles, *out, C.byref(rep), C.byref(err))
    rc, tree = _calltree(call)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), tree, _take_str(lib, err)


class MemoryPage(C.Structure):
    _fields_ = [("page", C.c_uint32), ("words", C.c_uint32), ("first", C.c_uint32), ("pad", C.c_uint32), ("loads", C.c_uint64),
                ("stores", C.c_uint64), ("pre_reads", C.c_uint64), ("pre_writes", C.c_uint64)]


class MemorySummary(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("cycles", "loads", "stores", "pre_reads", "pre_writes", "pre_calls", "words", "first_touches",
                                                "image_words", "image_words_accessed", "mem_init_rows", "sp_writes")] + \
               [(name, C.c_uint32) for name in ("sp_min", "sp_max", "text_base", "n_instr", "n_pages", "page_bytes", "shards_tallied",
                                                "shards_total")] + [("ms", C.c_float)]


MEMORY_LDS_PAGE_SLOTS = 256   # csrc/memreport.h LDS_PAGE_SLOTS: slots of a workgroup's page cache in the device pass


def _memory(call):
    """The memory report through call(first_touch, cap_instr, pages, cap_pages, summary) -> rc: once for the sizes, once for
    the tables.  Returns (rc, report), report = None when a call fails without a summary, else dict(summary, first_touch
    (numpy u64, one per instruction of the text), pages = [dict(page (byte address), words, first, loads, stores, pre_reads,
    pre_writes)] sorted by address)."""
    s = MemorySummary()
    rc = call(None, 0, None, 0, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    n_instr, n_pages = int(s.n_instr), int(s.n_pages)
    ft = np.zeros(max(n_instr, 1), np.uint64)
    pages = (MemoryPage * max(n_pages, 1))()
    rc = call(ft.ctypes.data_as(C.POINTER(C.c_uint64)), n_instr, pages, n_pages, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    summary = {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in MemorySummary._fields_}
    keys = [name for name, _ in MemoryPage._fields_ if name != "pad"]
    return rc, dict(summary=summary, first_touch=ft[:n_instr],
                    pages=[{k: int(getattr(pg, k)) for k in keys} for pg in pages[:min(n_pages, int(s.n_pages))]])


def execute_memory(elf: bytes, stdin=(), max_cycles=0):
    """Host-only memory report (dvt_execute_memory): page traffic, footprint, first touches per instruction and the stack span.
    Returns (rc, report dict as execute() gives it, memory dict as Prover.job_memory gives it or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)

    def call(*out):
        if err.value:
            lib.dvt_free(C.cast(err, C.c_void_p))
        return lib.dvt_execute_memory(elf, len(elf), bufs, len(stdin), max_cycles, *out, C.byref(rep), C.byref(err))
    rc, mem = _memory(call)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), mem, _take_str(lib, err)


# ---- watchpoints (csrc/watch.h)
DVT_WATCH_MAX_QUERIES, DVT_WATCH_MAX_KEEP, DVT_WATCH_SPAN = 16, 256, 4096
DVT_WATCH_PC, DVT_WATCH_REG, DVT_WATCH_MEM = 1, 2, 3
DVT_WATCH_LOAD, DVT_WATCH_STORE, DVT_WATCH_PRE_READ, DVT_WATCH_PRE_WRITE, DVT_WATCH_VALUE, DVT_WATCH_HIT_NO_VALUE = 1, 2, 4, 8, 16, 32
WATCH_EVERYWHERE = ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF))   # the window (from, to) that searches every position


class WatchQuery(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("kind", "flags", "lo", "hi", "mask", "want", "from_shard", "from_row", "to_shard", "to_row")]


class WatchHit(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("query", "shard", "row", "pc", "idx", "kind", "flags", "addr", "n_words", "before", "after",
                                                "rd_value", "rs1", "rs2", "prev_shard", "prev_clk")]


class WatchSummary(C.Structure):
    _fields_ = [("cycles", C.c_uint64)] + [(name, C.c_uint32) for name in ("n_queries", "cap_each", "shards_searched", "shards_total", "text_base",
                                                                           "n_instr", "span")] + [("ms", C.c_float)]


def _watch_query(kind, flags, lo, hi, mask, want, window):
    (fs, fr), (ts, tr) = window or WATCH_EVERYWHERE
    return dict(kind=kind, flags=flags, lo=lo, hi=hi, mask=mask, want=want, from_shard=fs, from_row=fr, to_shard=ts, to_row=tr)


def watch_pc(lo, hi=None, window=None):
    """the records whose pc lies in [lo, hi) (hi = None: the instruction at lo); window = ((shard, row), (shard, row)), `to` exclusive"""
    return _watch_query(DVT_WATCH_PC, 0, lo, lo + 4 if hi is None else hi, 0, 0, window)


def watch_reg(reg, value=None, mask=0xFFFFFFFF, window=None):
    """the records that write register `reg` (1..31); value: only those that write (value & mask)"""
    return _watch_query(DVT_WATCH_REG, 0 if value is None else DVT_WATCH_VALUE, reg, reg + 1, mask if value is not None else 0, value or 0, window)


def watch_mem(lo, hi=None, flags=DVT_WATCH_LOAD | DVT_WATCH_STORE | DVT_WATCH_PRE_READ | DVT_WATCH_PRE_WRITE, value=None, mask=0xFFFFFFFF, window=None):
    """the accesses of the words in [lo, hi) (hi = None: the word at lo) in the directions of flags; value: only the loads and
    stores that leave (value & mask) in the word"""
    return _watch_query(DVT_WATCH_MEM, flags | (0 if value is None else DVT_WATCH_VALUE), lo, lo + 4 if hi is None else hi,
                        mask if value is not None else 0, value or 0, window)


_HIT_KEYS = [name for name, _ in WatchHit._fields_]


def _watch(call, queries, keep):
    """The search through call(queries, n, cap_each, hits, totals, summary) -> rc.  Returns (rc, [dict(total, first = [hit dicts],
    last = [hit dicts])] per query or None when the call fails without lists, summary dict or None)."""
    n = len(queries)
    qs = (WatchQuery * max(n, 1))(*[WatchQuery(**q) for q in queries])
    hits = (WatchHit * max(2 * n * keep, 1))()
    totals = (C.c_uint64 * max(n, 1))()
    s = WatchSummary()
    rc = call(qs, n, keep, hits, totals, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None, None
    out = []
    for q in range(n):
        k = min(keep, int(totals[q]))
        lists = [[{name: int(getattr(hits[(2 * q + half) * keep + i], name)) for name in _HIT_KEYS} for i in range(k)] for half in (0, 1)]
        out.append(dict(total=int(totals[q]), first=lists[0], last=lists[1]))
    return rc, out, {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in WatchSummary._fields_}


def execute_watch(elf: bytes, stdin=(), queries=(), keep=16, max_cycles=0, log_shard=21):
    """Host-only watchpoints (dvt_execute_watch): the guest runs in shards of 2^log_shard cycles and every retired instruction
    is tested against the queries (watch_pc / watch_reg / watch_mem).  Returns (rc, report dict as execute() gives it, per query
    dict(total, first, last) as Prover.job_watch gives them or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)
    rc, found, _ = _watch(lambda *io: lib.dvt_execute_watch(elf, len(elf), bufs, len(stdin), max_cycles, log_shard, *io, C.byref(rep), C.byref(err)),
                          list(queries), keep)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), found, _take_str(lib, err)


# ---- snapshots (csrc/snapshot.h)
DVT_SNAP_MAX_RANGES, DVT_SNAP_MAX_WORDS, DVT_SNAP_SPAN = 16, 4096, 4096
(DVT_SNAP_INITIAL, DVT_SNAP_FROM_BEFORE, DVT_SNAP_FROM_AFTER, DVT_SNAP_LOAD, DVT_SNAP_STORE, DVT_SNAP_IMAGE, DVT_SNAP_NO_VALUE,
 DVT_SNAP_UNTOUCHED) = 1, 2, 4, 8, 16, 32, 64, 128
SNAP_EXIT = (0xFFFFFFFF, 0xFFFFFFFF)   # the position after the last record
REG_NAMES = ("zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1", "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "s2", "s3", "s4", "s5",
             "s6", "s7", "s8", "s9", "s10", "s11", "t3", "t4", "t5", "t6")


class SnapRange(C.Structure):
    _fields_ = [("lo", C.c_uint32), ("hi", C.c_uint32)]


class SnapCell(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("addr", "value", "flags", "shard", "row", "pc")]


class SnapFrame(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("fn_pc", "call_pc", "open_shard", "open_row", "ra", "pad")]


class SnapSummary(C.Structure):
    _fields_ = [("position", C.c_uint64), ("cycles", C.c_uint64)] + \
               [(name, C.c_uint32) for name in ("shard", "row", "pc", "depth", "n_frames", "unmatched_returns", "n_words", "no_value", "initial",
                                                "untouched", "shards_total", "text_base", "n_instr", "span")] + [("ms", C.c_float)]


def snap_range(addr, n_bytes=4):
    """the words that hold the bytes [addr, addr + n_bytes), as a (lo, hi) pair of word addresses"""
    return addr & ~3, (addr + max(n_bytes, 1) + 3) & ~3


_CELL_KEYS = [name for name, _ in SnapCell._fields_]
_FRAME_KEYS = [name for name, _ in SnapFrame._fields_ if name != "pad"]


def _snapshot(call, at, ranges, frames):
    """The snapshot through call(shard, row, ranges, n, regs, words, cap_words, frames, cap_frames, summary) -> rc.  Returns (rc,
    dict(summary, regs = 32 cell dicts, words = cell dicts in range order, frames = frame dicts innermost first) or None when
    the call fails without an answer)."""
    ranges = [tuple(r) for r in ranges]
    n_words = sum(max(0, (hi - lo) // 4) for lo, hi in ranges)
    rs = (SnapRange * max(len(ranges), 1))(*[SnapRange(lo, hi) for lo, hi in ranges])
    regs, words, fr, s = (SnapCell * 32)(), (SnapCell * max(n_words, 1))(), (SnapFrame * max(frames, 1))(), SnapSummary()
    rc = call(at[0], at[1], rs, len(ranges), regs, words, n_words, fr, frames, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    cell = lambda c: {name: int(getattr(c, name)) for name in _CELL_KEYS}
    summary = {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in SnapSummary._fields_}
    return rc, dict(summary=summary, regs=[cell(regs[k]) for k in range(32)], words=[cell(words[i]) for i in range(summary["n_words"])],
                    frames=[{name: int(getattr(fr[i], name)) for name in _FRAME_KEYS} for i in range(summary["n_frames"])])


def execute_snapshot(elf: bytes, stdin=(), at=SNAP_EXIT, ranges=(), frames=64, max_cycles=0, log_shard=21):
    """Host-only snapshot (dvt_execute_snapshot): the guest runs in shards of 2^log_shard cycles; the state before the record at
    `at` = (shard, row), SNAP_EXIT: after the last record (of a guest that traps: at the trap).  Returns (rc, report dict as
    execute() gives it, dict(summary, regs, words, frames) as Prover.job_snapshot gives it or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)
    rc, snap = _snapshot(lambda *io: lib.dvt_execute_snapshot(elf, len(elf), bufs, len(stdin), max_cycles, log_shard, *io, C.byref(rep), C.byref(err)),
                         at, ranges, frames)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), snap, _take_str(lib, err)


# ---- origins (csrc/origin.h)
DVT_ORIGIN_MAX_NODES, DVT_ORIGIN_MAX_EDGES, DVT_ORIGIN_MAX_DEPTH, DVT_ORIGIN_PASS_QUESTIONS, DVT_ORIGIN_SPAN = 1024, 8192, 64, 256, 4096
DVT_ORIGIN_NONE = 0xFFFFFFFF
DVT_ORIGIN_REG, DVT_ORIGIN_WORD = 1, 2
DVT_ORIGIN_FOLLOW_ADDR = 1
DVT_ORIGIN_OP, DVT_ORIGIN_LOAD, DVT_ORIGIN_STORE, DVT_ORIGIN_CALL, DVT_ORIGIN_SYSCALL = 1, 2, 3, 4, 5
DVT_ORIGIN_ROOT, DVT_ORIGIN_ADDR, DVT_ORIGIN_RS1, DVT_ORIGIN_RS2, DVT_ORIGIN_MEM = 0, 1, 2, 3, 4
DVT_ORIGIN_INITIAL, DVT_ORIGIN_IMAGE, DVT_ORIGIN_NO_VALUE, DVT_ORIGIN_CUT, DVT_ORIGIN_UNEXPANDED = 1, 2, 4, 8, 16


class OriginNode(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("shard", "row", "pc", "idx", "kind", "depth", "first_edge", "n_edges", "flags", "rd_value", "rs1", "rs2",
                                                "addr", "before", "after", "pad")]


class OriginEdge(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("from", "to", "role", "target", "value", "flags", "src_shard", "src_row")]


class OriginSummary(C.Structure):
    _fields_ = [("position", C.c_uint64), ("cycles", C.c_uint64)] + \
               [(name, C.c_uint32) for name in ("n_nodes", "n_edges", "depth", "cut", "unexpanded", "initial", "no_value", "questions", "levels", "passes",
                                                "shard", "row", "shards_total", "span")] + [("ms", C.c_float)]


def origin_reg(k):
    """the target of an origin call: register x_k (a number 1..31 or a name of REG_NAMES)"""
    return DVT_ORIGIN_REG, REG_NAMES.index(k) if isinstance(k, str) else int(k)


def origin_word(addr):
    """the target of an origin call: the word that holds the byte at addr"""
    return DVT_ORIGIN_WORD, addr & ~3


_NODE_KEYS = [name for name, _ in OriginNode._fields_ if name != "pad"]
_EDGE_KEYS = [name for name, _ in OriginEdge._fields_]


def _origin(call, at, target, follow_addr, depth, nodes, edges):
    """The slice through call(shard, row, what, target, flags, max_depth, nodes, cap_nodes, edges, cap_edges, summary) -> rc.
    Returns (rc, dict(summary, nodes = node dicts in discovery order, edges = edge dicts, edge 0 the root) or None when the call
    fails without an answer)."""
    ns, es, s = (OriginNode * max(nodes, 1))(), (OriginEdge * max(edges, 1))(), OriginSummary()
    rc = call(at[0], at[1], target[0], target[1], DVT_ORIGIN_FOLLOW_ADDR if follow_addr else 0, depth, ns, nodes, es, edges, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    summary = {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in OriginSummary._fields_}
    return rc, dict(summary=summary, nodes=[{name: int(getattr(ns[i], name)) for name in _NODE_KEYS} for i in range(summary["n_nodes"])],
                    edges=[{name: int(getattr(es[i], name)) for name in _EDGE_KEYS} for i in range(summary["n_edges"])])


def execute_origin(elf: bytes, stdin=(), at=SNAP_EXIT, target=(DVT_ORIGIN_REG, 10), follow_addr=False, depth=DVT_ORIGIN_MAX_DEPTH,
                   nodes=DVT_ORIGIN_MAX_NODES, edges=DVT_ORIGIN_MAX_EDGES, max_cycles=0, log_shard=21):
    """Host-only origin slice (dvt_execute_origin): the guest runs in shards of 2^log_shard cycles; where the value `target`
    (origin_reg() / origin_word()) holds before the record at `at` = (shard, row) comes from, SNAP_EXIT: after the last record
    (of a guest that traps: at the trap).  Returns (rc, report dict as execute() gives it, dict(summary, nodes, edges) as
    Prover.job_origin gives it or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)
    rc, got = _origin(lambda *io: lib.dvt_execute_origin(elf, len(elf), bufs, len(stdin), max_cycles, log_shard, *io, C.byref(rep), C.byref(err)),
                      at, target, follow_addr, depth, nodes, edges)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), got, _take_str(lib, err)


# ---- uses (csrc/uses.h)
DVT_USES_MAX_NODES, DVT_USES_MAX_DEFS, DVT_USES_MAX_EDGES, DVT_USES_MAX_DEPTH, DVT_USES_MAX_FAN, DVT_USES_DEFAULT_FAN = 1024, 4096, 8192, 64, 16, 8
DVT_USES_PASS_DEFS, DVT_USES_SPAN = 256, 4096
DVT_USES_NONE = 0xFFFFFFFF
DVT_USES_REG, DVT_USES_WORD = 1, 2
DVT_USES_FOLLOW_ADDR = 1
DVT_USES_OP, DVT_USES_LOAD, DVT_USES_STORE, DVT_USES_CALL, DVT_USES_SYSCALL = 1, 2, 3, 4, 5
DVT_USES_ADDR, DVT_USES_RS1, DVT_USES_RS2, DVT_USES_MEM = 1, 2, 3, 4
DVT_USES_LIVE_AT_EXIT, DVT_USES_TRUNCATED, DVT_USES_NO_VALUE, DVT_USES_CUT, DVT_USES_UNEXPANDED = 1, 2, 4, 8, 16


class UsesNode(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("shard", "row", "pc", "idx", "kind", "depth", "first_def", "n_defs", "flags", "rd_value", "rs1", "rs2",
                                                "addr", "before", "after", "pad")]


class UsesDef(C.Structure):
    _fields_ = [("n_uses", C.c_uint64)] + [(name, C.c_uint32) for name in ("node", "what", "target", "value", "flags", "next_shard", "next_row",
                                                                            "first_edge", "n_edges", "pad")]


class UsesEdge(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("def", "to", "role", "flags", "dst_shard", "dst_row")]


class UsesSummary(C.Structure):
    _fields_ = [("position", C.c_uint64), ("cycles", C.c_uint64), ("uses_total", C.c_uint64)] + \
               [(name, C.c_uint32) for name in ("n_nodes", "n_defs", "n_edges", "depth", "cut", "unexpanded", "truncated", "live_at_exit", "no_value", "dead",
                                                "levels", "passes", "shard", "row", "shards_total", "span")] + [("ms", C.c_float), ("pad", C.c_uint32)]


def uses_reg(k):
    """the target of a uses call: register x_k (a number 1..31 or a name of REG_NAMES)"""
    return DVT_USES_REG, REG_NAMES.index(k) if isinstance(k, str) else int(k)


def uses_word(addr):
    """the target of a uses call: the word that holds the byte at addr"""
    return DVT_USES_WORD, addr & ~3


def _uses(call, at, target, follow_addr, depth, fan, nodes, defs, edges):
    """The forward slice through call(shard, row, what, target, flags, max_depth, fan, nodes, cap_nodes, defs, cap_defs, edges,
    cap_edges, summary) -> rc.  Returns (rc, dict(summary, nodes = node dicts in discovery order, defs = definition dicts, defs[0]
    the root, edges = edge dicts) or None when the call fails without an answer)."""
    ns, ds, es, s = (UsesNode * max(nodes, 1))(), (UsesDef * max(defs, 1))(), (UsesEdge * max(edges, 1))(), UsesSummary()
    rc = call(at[0], at[1], target[0], target[1], DVT_USES_FOLLOW_ADDR if follow_addr else 0, depth, fan, ns, nodes, ds, defs, es, edges, C.byref(s))
    if rc not in (DVT_OK, DVT_ERR_GUEST):
        return rc, None
    summary = {name: (float if name == "ms" else int)(getattr(s, name)) for name, _ in UsesSummary._fields_ if name != "pad"}
    rows = lambda arr, cls, n: [{name: int(getattr(arr[i], name)) for name, _ in cls._fields_ if name != "pad"} for i in range(n)]
    return rc, dict(summary=summary, nodes=rows(ns, UsesNode, summary["n_nodes"]), defs=rows(ds, UsesDef, summary["n_defs"]),
                    edges=rows(es, UsesEdge, summary["n_edges"]))


def execute_uses(elf: bytes, stdin=(), at=SNAP_EXIT, target=(DVT_USES_REG, 10), follow_addr=False, depth=DVT_USES_MAX_DEPTH, fan=DVT_USES_DEFAULT_FAN,
                 nodes=DVT_USES_MAX_NODES, defs=DVT_USES_MAX_DEFS, edges=DVT_USES_MAX_EDGES, max_cycles=0, log_shard=21):
    """Host-only forward slice (dvt_execute_uses): the guest runs in shards of 2^log_shard cycles; who reads the value `target`
    (uses_reg() / uses_word()) holds from the record at `at` = (shard, row) on, and what those readers produce.  Returns (rc,
    report dict as execute() gives it, dict(summary, nodes, defs, edges) as Prover.job_uses gives it or None, error text)."""
    lib = load()
    rep, err, bufs = Report(), C.c_char_p(), _bufs(stdin)
    rc, got = _uses(lambda *io: lib.dvt_execute_uses(elf, len(elf), bufs, len(stdin), max_cycles, log_shard, *io, C.byref(rep), C.byref(err)),
                    at, target, follow_addr, depth, fan, nodes, defs, edges)
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), got, _take_str(lib, err)


# ---- divergence (csrc/diverge.h)
DVT_DIVERGE_SPAN, DVT_DIVERGE_MAX_KEEP, DVT_DIVERGE_MAX_WINDOW, DVT_DIVERGE_DEFAULT_WINDOW = 4096, 64, 16384, 4096
DVT_DIVERGE_BATCH_PAIRS = 1 << 20   # the header's default; a library may be built with another: summary["batch_pairs"] is the built value
DVT_DIV_NONE, DVT_DIVERGE_NO_REJOIN = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
DVT_DIV_RD, DVT_DIV_RS1, DVT_DIV_RS2, DVT_DIV_MEM = 1, 2, 4, 8
DVT_DIVERGE_REJOIN = 1
DVT_DIV_SPLIT, DVT_DIV_BAD, DVT_DIV_END_BOTH, DVT_DIV_END_A, DVT_DIV_END_B, DVT_DIV_LIMIT = 1, 2, 3, 4, 5, 6
DIV_REASONS = {1: "split", 2: "bad", 3: "end_both", 4: "end_a", 5: "end_b", 6: "limit"}
DIVERGE_ENTRY = (1, 0)   # the start of an execution


class DivergePos(C.Structure):
    _fields_ = [("shard", C.c_uint32), ("row", C.c_uint32)]


class DivergeRec(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("valid", "pc", "idx", "a", "b", "c", "m_prev", "pad")]


class DivergePair(C.Structure):
    _fields_ = [("k", C.c_uint64)] + [(name, C.c_uint32) for name in ("shard_a", "row_a", "shard_b", "row_b", "idx", "pc", "mask", "dir", "a_a", "b_a", "c_a",
                                                                       "m_a", "a_b", "b_b", "c_b", "m_b", "addr_a", "before_a", "after_a", "addr_b", "before_b",
                                                                       "after_b")]


class DivergeReg(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("n_diff", "first_diff", "last_diff", "last_write")] + [("live", C.c_uint32), ("pad", C.c_uint32)]


class DivergeSummary(C.Structure):
    _fields_ = [(name, C.c_uint64) for name in ("n_pairs", "n_data", "first_data", "last_data", "n_load_diffs", "n_store_diffs", "launched_pairs", "cycles_a",
                                                "cycles_b")] + \
               [(name, C.c_uint32) for name in ("reason", "mask", "stop_shard_a", "stop_row_a", "stop_shard_b", "stop_row_b", "rejoin_shard_a", "rejoin_row_a",
                                                "rejoin_shard_b", "rejoin_row_b", "rejoin_skip_a", "rejoin_skip_b", "n_kept", "span", "window", "batch_pairs")] + \
               [(name, DivergeRec) for name in ("stop_a", "stop_b", "prev_a", "prev_b")] + [("ms", C.c_float), ("pad2", C.c_uint32)]


_DIV_PAIR_KEYS = [name for name, _ in DivergePair._fields_]
_DIV_REG_KEYS = [name for name, _ in DivergeReg._fields_ if name != "pad"]
_DIV_REC_KEYS = [name for name, _ in DivergeRec._fields_ if name != "pad"]


def _diverge(call, start_a, start_b, max_pairs, rejoin, window, keep):
    """The report through call(start_a, start_b, max_pairs, flags, window, cap_each, first, last, regs, summary) -> rc.  Returns (rc,
    dict(summary, regs = 32 dicts, first, last = pair dicts) or None when the call fails without an answer).  In the summary the
    four records are dicts (or None where there is none)."""
    first, last, regs, s = (DivergePair * max(keep, 1))(), (DivergePair * max(keep, 1))(), (DivergeReg * 32)(), DivergeSummary()
    rc = call(DivergePos(*start_a), DivergePos(*start_b), max_pairs, DVT_DIVERGE_REJOIN if rejoin else 0, window, keep, first, last, regs, C.byref(s))
    if rc != DVT_OK:
        return rc, None
    summary = {}
    for name, kind in DivergeSummary._fields_:
        if name in ("pad", "pad2"):
            continue
        v = getattr(s, name)
        if kind is DivergeRec:
            summary[name] = {k: int(getattr(v, k)) for k in _DIV_REC_KEYS if k != "valid"} if v.valid else None
        else:
            summary[name] = float(v) if name == "ms" else int(v)
    n = summary["n_kept"]
    return rc, dict(summary=summary, regs=[{k: int(getattr(regs[r], k)) for k in _DIV_REG_KEYS} for r in range(32)],
                    first=[{k: int(getattr(first[i], k)) for k in _DIV_PAIR_KEYS} for i in range(n)],
                    last=[{k: int(getattr(last[i], k)) for k in _DIV_PAIR_KEYS} for i in range(n)])


def execute_diverge(elf: bytes, stdin_a: bytes, stdin_b: bytes, start_a=DIVERGE_ENTRY, start_b=DIVERGE_ENTRY, max_pairs=0, rejoin=False, window=0, keep=16,
                    max_cycles=0, log_shard=21):
    """Host-only divergence report (dvt_execute_diverge): the guest runs on stdin_a and on stdin_b (one buffer each; b"": none) in
    shards of 2^log_shard cycles, and the two record streams are compared pair by pair from the starts on (csrc/diverge.h).  A guest
    that traps or exits non-zero ends its stream there.  Returns (rc, (report dict of A, of B) as execute() gives them,
    dict(summary, regs, first, last) as Prover.job_diverge gives it or None, error text)."""
    lib = load()
    reps, err = (Report(), Report()), C.c_char_p()
    a, b = bytes(stdin_a), bytes(stdin_b)
    rc, got = _diverge(lambda *io: lib.dvt_execute_diverge(elf, len(elf), a, len(a), b, len(b), max_cycles, log_shard, *io, C.byref(reps[0]), C.byref(reps[1]),
                                                           C.byref(err)), start_a, start_b, max_pairs, rejoin, window, keep)
    return rc, tuple(dict(cycles=r.cycles, exit_code=r.exit_code, halted=bool(r.halted), unprovable=bool(r.unprovable)) for r in reps), got, _take_str(lib, err)


def exec_rate(elf: bytes, stdin=(), log_shard=21, trace=False) -> float:
    """guest cycles / second of the host executor alone (fast or trace mode)"""
    return float(load().dvt_debug_exec_rate(elf, len(elf), _bufs(stdin), len(stdin), log_shard, int(trace)))


def keep_plan(mode, free, total, reserve, full, tree, later, remaining=0, count_known=True, full_cap=-1, full_kept=0) -> int:
    """The admission rule of "keep_phase1" (dvt_debug_keep_plan; host only, no device): the DVT_KEEP_* tier of a shard that
    keeps `full` bytes in full and `tree` bytes as a tree, with `free` of `total` bytes free, `reserve` to stay free, and
    `remaining` later shards of at least `later` bytes each still to come"""
    return int(load().dvt_debug_keep_plan(mode, free, total, reserve, full, tree, later, remaining, int(bool(count_known)), full_cap, full_kept))


def p2_f64_selfcheck(n: int, seed: int) -> int:
    """FP64 Poseidon2 (host evaluation) against the integer permutation on n states: the number of differing words"""
    return int(load().dvt_debug_p2_f64_selfcheck(n, seed))


def p2_f64_sbox_check(n: int, seed: int):
    """FP64 S-box against x^7 mod p on n random inputs of its input range plus edge values:
    (mismatches, [max |x2|, max |x3|, max |x4|, max |x7|])"""
    mx = (C.c_double * 4)()
    bad = load().dvt_debug_p2_f64_sbox_check(n, seed, mx)
    return int(bad), [float(v) for v in mx]


def ntt_group_check(n: int, seed: int):
    """Radix-8 group arithmetic of the K1 passes (csrc/ntt_group.cuh) against integer arithmetic mod p on n random groups
    plus an edge grid: (mismatching outputs, {"dif" | "dif_unit" | "dit": [max |factor|, |product| of stages 0, 1, 2,
    max |value before the last reduction|, max |output|]})"""
    mx = [(C.c_double * 8)() for _ in range(3)]
    bad = load().dvt_debug_ntt_group_check(n, seed, *mx)
    return int(bad), {k: [float(v) for v in m] for k, m in zip(("dif", "dif_unit", "dit"), mx)}


def execute_io(elf: bytes, stdin=(), max_cycles=0):
    """execute() that also returns what the guest wrote to fds other than 3: (rc, report, public_values, stdout, error text)."""
    lib = load()
    pv, n, so, m, rep, err = u8p(), C.c_size_t(), u8p(), C.c_size_t(), Report(), C.c_char_p()
    rc = lib.dvt_execute_io(elf, len(elf), _bufs(stdin), len(stdin), max_cycles, C.byref(pv), C.byref(n), C.byref(so), C.byref(m), C.byref(rep), C.byref(err))
    out = C.string_at(pv, n.value) if pv else b""
    sout = C.string_at(so, m.value) if so else b""
    for ptr in (pv, so):
        if ptr:
            lib.dvt_free(C.cast(ptr, C.c_void_p))
    return rc, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted), unprovable=bool(rep.unprovable)), out, sout, _take_str(lib, err)


def stdin_from_json(circuit_type: str, json_bytes: bytes, auth_commitment=False) -> bytes:
    """The one SP1Stdin buffer the reference's host writes for `circuit_type` (src/main.rs:448-459:
    typed serde_json parse -> serde_cbor -> stdin.write(&Vec<u8>)).  Raises DvtError(DVT_ERR_INPUT) where the
    reference's typed parse fails ("Failed to read input")."""
    lib = load()
    out, n, err = u8p(), C.c_size_t(), C.c_char_p()
    rc = lib.dvt_stdin_from_json(circuit_type.encode(), json_bytes, len(json_bytes), int(bool(auth_commitment)), C.byref(out), C.byref(n), C.byref(err))
    if rc:
        raise DvtError(rc, _take_str(lib, err))
    b = C.string_at(out, n.value)
    lib.dvt_free(C.cast(out, C.c_void_p))
    return b


def verify(vk: bytes, proof: bytes, fri_queries=100, pow_bits=16):
    """Host-only verification of a core proof.  Returns (ok, exit_code, public_values, reason)."""
    lib = load()
    ec, pv, n, why = C.c_int32(), u8p(), C.c_size_t(), C.c_char_p()
    rc = lib.dvt_verify(vk, len(vk), proof, len(proof), fri_queries, pow_bits, C.byref(ec), C.byref(pv), C.byref(n), C.byref(why))
    out = C.string_at(pv, n.value) if pv else b""
    if pv:
        lib.dvt_free(C.cast(pv, C.c_void_p))
    return rc == DVT_OK, ec.value, out, _take_str(lib, why)


def _transcode(fn, vk, proof, fri_queries, pow_bits):
    lib = load()
    out, n, why = u8p(), C.c_size_t(), C.c_char_p()
    rc = fn(vk, len(vk), proof, len(proof), fri_queries, pow_bits, C.byref(out), C.byref(n), C.byref(why))
    reason = _take_str(lib, why)
    if rc:
        raise DvtError(rc, reason)
    b = C.string_at(out, n.value)
    lib.dvt_free(C.cast(out, C.c_void_p))
    return b


def proof_compact(vk: bytes, proof: bytes, fri_queries=100, pow_bits=16) -> bytes:
    """Host-only: the proof (a container, or one machine-level shard proof) with every shard in the compact form ("DVP2":
    shared Merkle paths sent once).  Raises DvtError(DVT_ERR_REJECTED, the verifier's text) when a shard's host part fails."""
    return _transcode(load().dvt_proof_compact, vk, proof, fri_queries, pow_bits)


def proof_expand(vk: bytes, proof: bytes, fri_queries=100, pow_bits=16) -> bytes:
    """Host-only: the inverse of proof_compact (every shard as "DVP1", the dropped siblings recomputed)."""
    return _transcode(load().dvt_proof_expand, vk, proof, fri_queries, pow_bits)


def compact_list_sweep(vk: bytes, proof: bytes, fri_queries=100, pow_bits=16):
    """Host-only test hook: every word of every node list of the compact shards of a container that verifies, changed by
    +1 mod p in turn.  Returns (words changed, changes that were still accepted)."""
    lib = load()
    n, acc, why = C.c_uint64(), C.c_uint64(), C.c_char_p()
    rc = lib.dvt_debug_compact_list_sweep(vk, len(vk), proof, len(proof), fri_queries, pow_bits, C.byref(n), C.byref(acc), C.byref(why))
    reason = _take_str(lib, why)
    if rc:
        raise DvtError(rc, reason)
    return n.value, acc.value


def multipath_nodes(depth: int, indices):
    """Host-only: the (level, index) pairs a compact proof lists for a tree of 2^depth leaves queried at `indices`, in order."""
    lib = load()
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    n = C.c_size_t()
    rc = lib.dvt_stage_multipath_nodes(depth, idx.ctypes.data_as(u32p), idx.size, None, 0, C.byref(n))
    if rc:
        raise DvtError(rc, "dvt_stage_multipath_nodes")
    out = np.zeros((max(n.value, 1), 2), np.uint32)
    lib.dvt_stage_multipath_nodes(depth, idx.ctypes.data_as(u32p), idx.size, out.ctypes.data_as(u32p), n.value, C.byref(n))
    return [(int(a), int(b)) for a, b in out[:n.value]]


def split_container(proof: bytes):
    """The parts of a core proof ("DVC3" container, csrc/proof.h) -> (exit_code, public value bytes, [shard proof bytes])."""
    w = np.frombuffer(proof, np.uint32)
    assert w[0] == 0x33435644
    n, ec, pvl = int(w[1]), int(w[2]), int(w[3])
    at = 4 + (pvl + 3) // 4
    shards = []
    for _ in range(n):
        shards.append(w[at + 1:at + 1 + int(w[at])].tobytes())
        at += 1 + len(shards[-1]) // 4
    assert at == len(w)
    return ec, w[4:4 + (pvl + 3) // 4].tobytes()[:pvl], shards


def _parse_blob(w):
    nch = int(w[0])
    meta = w[1:1 + 4 * nch].reshape(nch, 4)
    at = 1 + 4 * nch
    npub = int(w[at])
    pubs = w[at + 1:at + 1 + npub].copy()
    at += 1 + npub
    chips = []
    for cid, lg, mw, pw in meta:
        h = 1 << int(lg)
        main = w[at:at + int(mw) * h].reshape(int(mw), h)
        at += int(mw) * h
        prep = w[at:at + int(pw) * h].reshape(int(pw), h)
        at += int(pw) * h
        chips.append(dict(chip_id=int(cid), log_n=int(lg), main=main, prep=prep))
    assert at == len(w)
    return chips, pubs


def rv32_debug_traces(elf: bytes, stdin=(), log_shard=0, shard=0):
    """Host-only: the traces the prover would commit for shard `shard` (0-based) of the run cut at
    2^log_shard cycles.  Returns (chips, pubs, n_shards); chips = list of dict(chip_id, log_n, main, prep)."""
    lib = load()
    blob, n, err, ns = u32p(), C.c_size_t(), C.c_char_p(), C.c_uint32()
    rc = lib.dvt_rv32_debug_traces(elf, len(elf), _bufs(stdin), len(stdin), log_shard, shard, C.byref(ns), C.byref(blob), C.byref(n), C.byref(err))
    if rc:
        raise DvtError(rc, _take_str(lib, err))
    w = np.ctypeslib.as_array(blob, shape=(n.value,)).copy()
    lib.dvt_free(C.cast(blob, C.c_void_p))
    chips, pubs = _parse_blob(w)
    return chips, pubs, ns.value


HEADER_WORDS = 13   # main-trace Merkle root (8) + public values (5): dvt_rv32_header_words()


def rv32_challenges(vk: bytes, headers):
    """Host-only: the LogUp challenges common to all shards, from their 13-word headers (in shard order)."""
    lib = load()
    h = np.ascontiguousarray(headers, dtype=np.uint32).reshape(-1, HEADER_WORDS)
    out = np.zeros(8, np.uint32)
    rc = lib.dvt_rv32_challenges(vk, len(vk), h.ctypes.data_as(u32p), h.shape[0], out.ctypes.data_as(u32p))
    if rc:
        raise DvtError(rc, "dvt_rv32_challenges")
    return out


def _traces(traces):
    """traces: list of (chip_id, ndarray [width][height] uint32 canonical)."""
    arr = (HostTrace * max(len(traces), 1))()
    keep = []
    for i, (cid, m) in enumerate(traces):
        m = np.ascontiguousarray(m, dtype=np.uint32)
        h = m.shape[1]
        lg = int(h).bit_length() - 1
        assert 1 << lg == h
        keep.append(m)
        arr[i] = HostTrace(cid, lg, m.ctypes.data_as(u32p))
    return arr, keep


def machine_verify(vk: bytes, proof: bytes, fri_queries=100, pow_bits=16):
    """Host-only verification.  Returns (ok, reason)."""
    lib = load()
    reason = C.c_char_p()
    rc = lib.dvt_machine_verify(vk, len(vk), proof, len(proof), fri_queries, pow_bits, C.byref(reason))
    why = reason.value.decode() if reason.value else ""
    if reason.value:
        lib.dvt_free(C.cast(reason, C.c_void_p))
    return rc == DVT_OK, why


class Prover:
    """Owns one dvt_prover handle: one GPU, or with "devices": [d0, d1, ...] in the cfg one device member per entry."""

    def __init__(self, cfg=None):
        """cfg: the handle's config as a JSON string, or as a dict of its keys."""
        if isinstance(cfg, dict):
            cfg = json.dumps(cfg)
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.dvt_prover_create(cfg.encode() if cfg else None, C.byref(h))
        if rc:
            raise DvtError(rc, self.lib.dvt_last_error(None).decode())
        self.h = h

    def close(self):
        if self.h:
            self.lib.dvt_prover_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc:
            raise DvtError(rc, self.lib.dvt_last_error(self.h).decode())

    def sync(self):
        self.check(self.lib.dvt_sync(self.h))

    def stream_ptr(self):
        return self.lib.dvt_stream(self.h)

    def device_count(self):
        """device members of the handle"""
        return int(self.lib.dvt_prover_device_count(self.h))

    def device(self, member):
        """HIP device index of a member, -1 out of range"""
        return int(self.lib.dvt_prover_device(self.h, member))

    # ---- stage-level helpers over torch int32 CUDA tensors (device memory plumbing only)
    def to_internal(self, t):
        self.check(self.lib.dvt_dev_to_internal(self.h, t.data_ptr(), t.numel()))

    def from_internal(self, t):
        self.check(self.lib.dvt_dev_from_internal(self.h, t.data_ptr(), t.numel()))

    def coset_lde(self, t_in, t_out, width, log_n, shift_mode=0, scratch=None):
        assert t_in.numel() == width << log_n and t_out.numel() == width << (log_n + 1)
        assert scratch is None or scratch.numel() >= width << log_n
        self.check(self.lib.dvt_stage_coset_lde(self.h, t_in.data_ptr(), scratch.data_ptr() if scratch is not None else None,
                                                t_out.data_ptr(), width, log_n, shift_mode))

    def merkle_commit(self, mats, t_digests):
        """mats: list of (tensor [width][height], width, log_height)."""
        arr = (DevMatrix * len(mats))()
        for i, (t, w, lh) in enumerate(mats):
            assert t.numel() == w << lh
            arr[i] = DevMatrix(t.data_ptr(), w, lh)
        need = self.lib.dvt_merkle_digest_words(arr, len(mats))
        assert t_digests.numel() >= need
        self.check(self.lib.dvt_stage_merkle_commit(self.h, arr, len(mats), t_digests.data_ptr()))
        return need

    def poseidon2_permute(self, t_states):
        assert t_states.numel() % 16 == 0
        self.check(self.lib.dvt_stage_poseidon2_permute(self.h, t_states.data_ptr(), t_states.numel() // 16))

    def fri_fold(self, t_v, t_out, beta, log_m, t_ro=None):
        assert t_v.numel() == 4 << log_m and t_out.numel() == 2 << log_m
        b = (C.c_uint32 * 4)(*[int(x) for x in beta])
        self.check(self.lib.dvt_stage_fri_fold(self.h, t_v.data_ptr(), t_out.data_ptr(), t_ro.data_ptr() if t_ro is not None else None, b, log_m))

    def logup_running_sum(self, t_totals, t_phi, log_n):
        """K4 tail: t_totals [4][2^log_n] (overwritten by its prefix sums) -> t_phi; returns the cumulative sum (canonical)."""
        assert t_totals.numel() == 4 << log_n and t_phi.numel() == 4 << log_n
        cum = (C.c_uint32 * 4)()
        self.check(self.lib.dvt_stage_logup_running_sum(self.h, t_totals.data_ptr(), t_phi.data_ptr(), log_n, cum))
        return list(cum)

    def open(self, mats, z):
        """K6: mats = list of (tensor [width][height], width, log_height) of one height; returns [columns][2][4] canonical
        words: each column's value at z and at z * w_n."""
        arr = (DevMatrix * len(mats))()
        for i, (t, w, lh) in enumerate(mats):
            assert t.numel() == w << lh
            arr[i] = DevMatrix(t.data_ptr(), w, lh)
        ncols = sum(w for _, w, _ in mats)
        out = np.zeros((max(ncols, 1), 2, 4), np.uint32)
        zz = (C.c_uint32 * 4)(*[int(x) for x in z])
        self.check(self.lib.dvt_stage_open(self.h, arr, len(mats), zz, out.ctypes.data_as(u32p)))
        return out[:ncols]

    def reduced_opening(self, cols, n_two, log_m, alpha, open_local, open_next, zeta, t_out):
        """K7: cols = list of device columns (tensors of 2^log_m words), the first n_two opened at two points;
        open_local [n_all][4] / open_next [n_two][4] canonical; t_out [2^log_m][4]."""
        assert all(t.numel() == 1 << log_m for t in cols) and t_out.numel() == 4 << log_m
        n_all = len(cols)
        ptrs = (C.c_void_p * max(n_all, 1))(*[t.data_ptr() for t in cols])
        ol = np.ascontiguousarray(np.asarray(open_local, np.uint32).reshape(-1, 4)) if n_all else np.zeros((1, 4), np.uint32)
        on = np.ascontiguousarray(np.asarray(open_next, np.uint32).reshape(-1, 4)) if n_two else np.zeros((1, 4), np.uint32)
        assert ol.shape[0] >= n_all and on.shape[0] >= n_two
        a = (C.c_uint32 * 4)(*[int(x) for x in alpha])
        ze = (C.c_uint32 * 4)(*[int(x) for x in zeta])
        self.check(self.lib.dvt_stage_reduced_opening(self.h, ptrs, n_two, n_all, log_m, a, ol.ctypes.data_as(u32p),
                                                      on.ctypes.data_as(u32p), ze, t_out.data_ptr()))

    def pow_grind(self, state, pos, bits):
        """K9: the smallest proof-of-work witness for 16 canonical state words, the witness in word pos."""
        st = (C.c_uint32 * 16)(*[int(x) for x in state])
        w = C.c_uint32()
        self.check(self.lib.dvt_stage_pow_grind(self.h, st, pos, bits, C.byref(w)))
        return w.value

    def perm(self, machine, chip, t_main, t_prep, log_n, pubs, perm_alpha, beta, t_perm, path="default"):
        """K4 of one chip: device matrices in Montgomery form (t_prep / t_perm None when the width is 0); the batch
        columns and phi go to t_perm; returns the cumulative sum (canonical)."""
        u4 = lambda v: (C.c_uint32 * 4)(*[int(x) for x in v])
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        cum = (C.c_uint32 * 4)()
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.check(self.lib.dvt_stage_perm(self.h, machine.encode(), chip, ptr(t_main), ptr(t_prep), log_n, pv, u4(perm_alpha), u4(beta),
                                           PATHS[path], ptr(t_perm), cum))
        return list(cum)

    def quotient(self, machine, chip, t_main_lde, t_prep_lde, t_perm_lde, log_n, pubs, perm_alpha, beta, alpha, cum, t_out,
                 path="default", selectors="table"):
        """K5 of one chip: LDEs in Montgomery form (None when the width is 0) -> t_out [2][4][2^log_n]."""
        u4 = lambda v: (C.c_uint32 * 4)(*[int(x) for x in v])
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        ptr = lambda t: t.data_ptr() if t is not None else None
        assert t_out.numel() == 8 << log_n
        self.check(self.lib.dvt_stage_quotient(self.h, machine.encode(), chip, ptr(t_main_lde), ptr(t_prep_lde), ptr(t_perm_lde), log_n,
                                               pv, u4(perm_alpha), u4(beta), u4(alpha), u4(cum), PATHS[path], SELECTORS[selectors],
                                               t_out.data_ptr()))

    def stage_check_constraints(self, machine, chip, t_main, t_prep, log_n, pubs, xi, n_constraints=None):
        """Trace-row check of one chip: device matrices in Montgomery form (t_prep None when the width is 0), xi = 4
        canonical words.  Returns (dict(violations, first_row, first_constraint), counts); counts is a uint32 array of
        n_constraints words (rows violating each unit), or None when n_constraints is None."""
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        x4 = (C.c_uint32 * 4)(*[int(x) for x in xi])
        counts = np.zeros(max(n_constraints, 1), np.uint32) if n_constraints is not None else None
        r = CheckResult()
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.check(self.lib.dvt_stage_check_constraints(self.h, machine.encode(), chip, ptr(t_main), ptr(t_prep), log_n, pv, x4,
                                                        counts.ctypes.data_as(u32p) if counts is not None else None, C.byref(r)))
        return (dict(violations=int(r.violations), first_row=int(r.first_row), first_constraint=int(r.first_constraint)),
                counts[:n_constraints] if counts is not None else None)

    def stage_bus_sums(self, machine, chip, t_main, t_prep, log_n, pubs, perm_alpha, beta):
        """The chip's signed LogUp terms summed over the rows, per bus: a [CHECK_BUSES][4] array of canonical words."""
        u4 = lambda v: (C.c_uint32 * 4)(*[int(x) for x in v])
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        out = np.zeros((CHECK_BUSES, 4), np.uint32)
        ptr = lambda t: t.data_ptr() if t is not None else None
        self.check(self.lib.dvt_stage_bus_sums(self.h, machine.encode(), chip, ptr(t_main), ptr(t_prep), log_n, pv, u4(perm_alpha), u4(beta),
                                               out.ctypes.data_as(u32p)))
        return out

    def _hunt_cells(self, call, main_w, deltas, row_count, want_map):
        dl = np.ascontiguousarray(deltas, dtype=np.uint32)
        counts = np.zeros((main_w, max(dl.size, 1)), np.uint32)
        fmap = np.zeros((max(dl.size, 1), main_w, max(row_count, 1)), np.uint8) if want_map else None
        self.check(call(dl.ctypes.data_as(u32p), dl.size, counts.ctypes.data_as(u32p), fmap.ctypes.data_as(u8p) if want_map else None))
        return counts[:, :dl.size], (fmap[:dl.size, :, :row_count] if want_map else None)

    def _hunt_pairs(self, call, deltas, cols, cap):
        dl = np.ascontiguousarray(deltas, dtype=np.uint32)
        cl = np.ascontiguousarray(cols, dtype=np.uint32) if cols is not None else None
        arr = (Escape * max(cap, 1))()
        n_rep, n_tried = C.c_uint64(), C.c_uint64()
        self.check(call(dl.ctypes.data_as(u32p), dl.size, cl.ctypes.data_as(u32p) if cl is not None else None, cl.size if cl is not None else 0,
                        arr, cap, C.byref(n_rep), C.byref(n_tried)))
        return dict(reported=_escapes(arr, min(int(n_rep.value), cap)), n_reported=int(n_rep.value), n_tried=int(n_tried.value))

    def stage_hunt_cells(self, machine, chip, t_main, t_prep, log_n, pubs, main_w, deltas, row_first=0, row_count=None, seed=1,
                         max_evals=0, want_map=True):
        """Single-cell forgeries of one chip table (dvt_stage_hunt_cells; matrices as stage_check_constraints takes them).
        Returns (free_counts [main_w][n_deltas], free_map [n_deltas][main_w][row_count] of 0 / 1 or None): where the change
        of a cell by a delta escapes every constraint and the LogUp multiset.  A table that is not honest raises
        DvtError(DVT_ERR_REJECTED)."""
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = (1 << log_n) - row_first if row_count is None else row_count
        call = lambda dl, nd, counts, fmap: self.lib.dvt_stage_hunt_cells(self.h, machine.encode(), chip, ptr(t_main), ptr(t_prep), log_n, pv, seed,
                                                                         dl, nd, row_first, rc, max_evals, counts, fmap)
        return self._hunt_cells(call, main_w, deltas, rc, want_map)

    def stage_hunt_pairs(self, machine, chip, t_main, t_prep, log_n, pubs, deltas, cols=None, adjacent=False, row_first=0, row_count=None,
                         seed=1, max_evals=0, cap=4096):
        """Two-cell forgeries of one chip table (dvt_stage_hunt_pairs).  Returns dict(reported, n_reported, n_tried): reported
        = at most cap dicts(row, n_cells, col, row_off, delta, alone) sorted by (row, col, delta): pairs that escape although
        one of their changes alone is caught."""
        pv = (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = (1 << log_n) - row_first if row_count is None else row_count
        call = lambda dl, nd, cl, nc, arr, cp, a, b: self.lib.dvt_stage_hunt_pairs(self.h, machine.encode(), chip, ptr(t_main), ptr(t_prep), log_n, pv,
                                                                                  seed, dl, nd, cl, nc, int(adjacent), row_first, rc, max_evals,
                                                                                  arr, cp, a, b)
        return self._hunt_pairs(call, deltas, cols, cap)

    def hunt_join(self, machine, windows, deltas, supply=(), seed=1, max_evals=0, cap_records=1 << 16, cap_absorbed=1 << 16, log_slots=0,
                  cap_cells=1 << 16):
        """The join hunt over windows of several chip tables (dvt_stage_hunt_join_*): two-cell forgeries whose halves lie in
        different tables or in distant rows, and single cells that a supply table absorbs.  windows: dicts(tag, chip, main,
        prep, log_n, pubs[, row_first, row_count, cols]); supply: dicts(chip, main, prep, log_n, pubs); matrices as
        stage_check_constraints takes them.  Returns dict(summary, groups, absorbed): summary = the fields of
        dvt_join_summary, with DVT_JOIN_TRUNC_OUTPUT also set when more cells exist than cap_cells; groups = a list of
        [side 0, side 1], each a list of dicts(tag, chip, col, row, delta) in the result's order; absorbed = such dicts."""
        dl = np.ascontiguousarray(deltas, dtype=np.uint32)
        ptr = lambda t: t.data_ptr() if t is not None else None
        pubv = lambda pubs: (C.c_uint32 * max(len(pubs), 1))(*[int(x) for x in pubs])
        h = C.c_void_p()
        self.check(self.lib.dvt_stage_hunt_join_new(self.h, machine.encode(), seed, dl.ctypes.data_as(u32p), dl.size, cap_records, cap_absorbed,
                                                    log_slots, C.byref(h)))
        try:
            # (the library keeps the supply matrices' device pointers until the first add: `supply` holds the tensors until then)
            supply = list(supply)
            for s in supply:
                self.check(self.lib.dvt_stage_hunt_join_supply(self.h, h, s["chip"], ptr(s["main"]), ptr(s.get("prep")), s["log_n"], pubv(s["pubs"])))
            for w in windows:
                first = w.get("row_first", 0)
                count = w.get("row_count")
                count = (1 << w["log_n"]) - first if count is None else count
                cl = np.ascontiguousarray(w["cols"], dtype=np.uint32) if w.get("cols") is not None else None
                self.check(self.lib.dvt_stage_hunt_join_add(self.h, h, w["tag"], w["chip"], ptr(w["main"]), ptr(w.get("prep")), w["log_n"],
                                                            pubv(w["pubs"]), first, count, cl.ctypes.data_as(u32p) if cl is not None else None,
                                                            cl.size if cl is not None else 0, max_evals))
            sm = JoinSummary()
            self.check(self.lib.dvt_stage_hunt_join_match(self.h, h, C.byref(sm)))
            cells, soaked = (JoinCell * max(cap_cells, 1))(), (JoinCell * max(cap_absorbed, 1))()
            n_cells, n_soaked = C.c_size_t(), C.c_size_t()
            self.check(self.lib.dvt_stage_hunt_join_result(self.h, h, cells, cap_cells, C.byref(n_cells), soaked, cap_absorbed, C.byref(n_soaked)))
        finally:
            self.lib.dvt_stage_hunt_join_free(self.h, h)
        return _join_result(sm, cells, n_cells.value, cap_cells, soaked, n_soaked.value, cap_absorbed)

    def hunt_join_job(self, pk, job, windows, deltas, supply_chips=(0, 1, 3), cols=None, seed=1, max_evals=0, cap_records=1 << 16,
                      cap_absorbed=1 << 16, log_slots=0, cap_cells=1 << 16):
        """The join hunt over windows of a prepared job's tables (dvt_rv32_hunt_join_job).  windows: tuples (shard, chip[,
        row_first[, row_count]]), row_count 0 / missing = to the end of the table; the tag of a cell is its shard.
        supply_chips: the supply tables, taken from the first window's shard (default program, byte, mem_image).  cols: None, or
        one list of columns (or None = all) per window.  Returns what hunt_join returns.  Windows on shards of several device
        members raise DvtError(DVT_ERR_UNSUPPORTED).  The job is left as found."""
        dl = np.ascontiguousarray(deltas, dtype=np.uint32)
        ws = (JoinWindow * max(len(windows), 1))(*[JoinWindow(*(tuple(w) + (0, 0))[:4]) for w in windows])
        sc = np.ascontiguousarray(list(supply_chips), dtype=np.uint32)
        counts = np.ascontiguousarray([len(c) if c is not None else 0 for c in cols], dtype=np.uint32) if cols is not None else None
        flat = np.ascontiguousarray([x for c in cols if c is not None for x in c] + [0], dtype=np.uint32) if cols is not None else None
        sm = JoinSummary()
        cells, soaked = (JoinCell * max(cap_cells, 1))(), (JoinCell * max(cap_absorbed, 1))()
        n_cells, n_soaked = C.c_size_t(), C.c_size_t()
        self.check(self.lib.dvt_rv32_hunt_join_job(self.h, pk, job, ws, len(windows), sc.ctypes.data_as(u32p) if sc.size else None, sc.size, seed,
                                                   dl.ctypes.data_as(u32p), dl.size, flat.ctypes.data_as(u32p) if flat is not None else None,
                                                   counts.ctypes.data_as(u32p) if counts is not None else None, max_evals, cap_records, cap_absorbed,
                                                   log_slots, C.byref(sm), cells, cap_cells, C.byref(n_cells), soaked, cap_absorbed, C.byref(n_soaked)))
        return _join_result(sm, cells, n_cells.value, cap_cells, soaked, n_soaked.value, cap_absorbed)

    def hunt_shard(self, pk, job, shard, chip, deltas, pairs=False, cols=None, adjacent=False, row_first=0, row_count=None,
                   seed=1, max_evals=0, cap=4096, want_map=True):
        """The same two hunts on chip `chip` of a shard of a prepared job (dvt_rv32_hunt_shard): what stage_hunt_cells
        (pairs False) or stage_hunt_pairs (pairs True) returns."""
        main_w, log_n = self.job_shard_chip_shape(job, shard, chip)
        rc = (1 << log_n) - row_first if row_count is None else row_count
        if pairs:
            call = lambda dl, nd, cl, nc, arr, cp, a, b: self.lib.dvt_rv32_hunt_shard(self.h, pk, job, shard, chip, seed, dl, nd, 1, cl, nc, int(adjacent),
                                                                                     row_first, rc, max_evals, None, None, arr, cp, a, b)
            return self._hunt_pairs(call, deltas, cols, cap)
        call = lambda dl, nd, counts, fmap: self.lib.dvt_rv32_hunt_shard(self.h, pk, job, shard, chip, seed, dl, nd, 0, None, 0, 0, row_first, rc,
                                                                        max_evals, counts, fmap, None, 0, None, None)
        return self._hunt_cells(call, main_w, deltas, rc, want_map)

    # ---- machine level
    def verify(self, vk: bytes, proof: bytes, fri_queries=100, pow_bits=16):
        """capi.verify with the query part on this handle's GPU.  Returns (ok, exit_code, public_values, reason); a device
        failure raises."""
        lib = self.lib
        ec, pv, n, why = C.c_int32(), u8p(), C.c_size_t(), C.c_char_p()
        rc = lib.dvt_prover_verify(self.h, vk, len(vk), proof, len(proof), fri_queries, pow_bits, C.byref(ec), C.byref(pv), C.byref(n), C.byref(why))
        out = C.string_at(pv, n.value) if pv else b""
        if pv:
            lib.dvt_free(C.cast(pv, C.c_void_p))
        reason = _take_str(lib, why)
        if rc == DVT_ERR_DEVICE:
            self.check(rc)
        return rc == DVT_OK, ec.value, out, reason

    def machine_verify(self, vk: bytes, proof: bytes, fri_queries=100, pow_bits=16):
        """capi.machine_verify with the query part on this handle's GPU.  Returns (ok, reason); a device failure raises."""
        reason = C.c_char_p()
        rc = self.lib.dvt_prover_machine_verify(self.h, vk, len(vk), proof, len(proof), fri_queries, pow_bits, C.byref(reason))
        why = reason.value.decode() if reason.value else ""
        if reason.value:
            self.lib.dvt_free(C.cast(reason, C.c_void_p))
        if rc == DVT_ERR_DEVICE:
            self.check(rc)
        return rc == DVT_OK, why

    def verify_times(self):
        """The last verify / machine_verify of this handle: milliseconds of the host part, flattening, uploads, kernels,
        downloads and waiting, then permutations, launches and chunks."""
        out = (C.c_double * 9)()
        self.check(self.lib.dvt_prover_verify_times(self.h, out))
        keys = ("host_ms", "flatten_ms", "upload_ms", "kernels_ms", "download_ms", "wait_ms", "permutations", "launches", "chunks")
        return dict(zip(keys, [float(x) for x in out]))

    def stage_sponge_rows(self, vectors):
        """Digests [n][8] (canonical) of n canonical word vectors: the sponge kernel of the device verifier."""
        lens = np.array([len(v) for v in vectors], np.uint32)
        words = np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint32) for v in vectors]) if len(vectors) else np.zeros(0, np.uint32))
        out = np.zeros((len(vectors), 8), np.uint32)
        self.check(self.lib.dvt_stage_sponge_rows(self.h, words.ctypes.data_as(u32p), lens.ctypes.data_as(u32p), len(vectors), out.ctypes.data_as(u32p)))
        return out

    def stage_verify_paths(self, chains):
        """chains: dicts with start [8], depth, leaf, siblings [depth][8], root [8] and optionally inject [depth][8] with
        inject_at [depth] (canonical words).  Returns the ok-bytes: the path kernel of the device verifier."""
        arr = (PathChain * len(chains))()
        keep = []

        def ptr(a, dt, ct):
            a = np.ascontiguousarray(np.asarray(a, dt).reshape(-1))
            if a.size == 0:
                a = np.zeros(1, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))

        for i, c in enumerate(chains):
            arr[i].start = ptr(c["start"], np.uint32, C.c_uint32)
            arr[i].depth, arr[i].leaf = int(c["depth"]), int(c["leaf"])
            arr[i].siblings = ptr(c["siblings"], np.uint32, C.c_uint32)
            arr[i].root = ptr(c["root"], np.uint32, C.c_uint32)
            if c.get("inject") is not None:
                arr[i].inject = ptr(c["inject"], np.uint32, C.c_uint32)
                arr[i].inject_at = ptr(c["inject_at"], np.uint8, C.c_uint8)
        ok = np.zeros(len(chains), np.uint8)
        self.check(self.lib.dvt_stage_verify_paths(self.h, arr, len(chains), ok.ctypes.data_as(u8p)))
        return ok

    def verify_multipath(self, depth, leaf_index, leaf_digest, nodes, root, inject=None, inject_at=None):
        """The tree kernel of the device verifier on one tree: n queries at leaf_index [n] with leaf_digest [n][8], the listed
        nodes [k][8] in multipath_nodes' order, optionally inject [depth][n][8] with inject_at [depth] (canonical words).
        Returns ok (bool)."""
        keep = []

        def ptr(a, dt, ct):
            a = np.ascontiguousarray(np.asarray(a, dt).reshape(-1))
            if a.size == 0:
                a = np.zeros(1, dt)
            keep.append(a)
            return a.ctypes.data_as(C.POINTER(ct))

        n = len(leaf_index)
        nodes = np.asarray(nodes, np.uint32).reshape(-1, 8)
        ok = np.zeros(1, np.uint8)
        self.check(self.lib.dvt_stage_verify_multipath(
            self.h, depth, ptr(leaf_index, np.uint32, C.c_uint32), ptr(leaf_digest, np.uint32, C.c_uint32), n,
            ptr(inject_at, np.uint8, C.c_uint8) if inject_at is not None else None,
            ptr(inject, np.uint32, C.c_uint32) if inject is not None else None,
            ptr(nodes, np.uint32, C.c_uint32), nodes.shape[0], ptr(root, np.uint32, C.c_uint32), ok.ctypes.data_as(u8p)))
        return bool(ok[0])

    def machine_setup(self, machine: str, prep):
        arr, keep = _traces(prep)
        pk, vk, n = C.c_void_p(), u8p(), C.c_size_t()
        self.check(self.lib.dvt_machine_setup(self.h, machine.encode(), arr, len(prep), C.byref(pk), C.byref(vk), C.byref(n)))
        vkb = bytes(bytearray(vk[: n.value]))
        self.lib.dvt_free(C.cast(vk, C.c_void_p))
        return pk, vkb

    def pk_free(self, pk):
        self.lib.dvt_pk_free(self.h, pk)

    def machine_prove(self, pk, main, pubs):
        arr, keep = _traces(main)
        pv = np.ascontiguousarray(pubs, dtype=np.uint32)
        out, n = u8p(), C.c_size_t()
        self.check(self.lib.dvt_machine_prove(self.h, pk, arr, len(main), pv.ctypes.data_as(u32p), pv.size, C.byref(out), C.byref(n)))
        b = C.string_at(out, n.value)
        self.lib.dvt_free(C.cast(out, C.c_void_p))
        return b

    # ---- the reference's boundary (src/main.rs:461-474)
    def setup(self, elf: bytes):
        pk, vk, n = C.c_void_p(), u8p(), C.c_size_t()
        self.check(self.lib.dvt_setup(self.h, elf, len(elf), C.byref(pk), C.byref(vk), C.byref(n)))
        vkb = C.string_at(vk, n.value)
        self.lib.dvt_free(C.cast(vk, C.c_void_p))
        return pk, vkb

    def prove_core(self, pk, stdin=()):
        out, n, rep = u8p(), C.c_size_t(), Report()
        self.check(self.lib.dvt_prove_core(self.h, pk, _bufs(stdin), len(stdin), C.byref(out), C.byref(n), C.byref(rep)))
        b = C.string_at(out, n.value)
        self.lib.dvt_free(C.cast(out, C.c_void_p))
        return b, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted))

    def prepare(self, pk, stdin=(), first=0, stride=1):
        """the executor pipeline (fast pass, traced re-execution of the owned shards first, first + stride, ...,
        upload, phase 1 on the GPU); returns (job handle, report)"""
        job, rep = C.c_void_p(), Report()
        self.check(self.lib.dvt_rv32_prepare_part(self.h, pk, _bufs(stdin), len(stdin), first, stride, C.byref(job), C.byref(rep)))
        return job, dict(cycles=rep.cycles, exit_code=rep.exit_code, halted=bool(rep.halted))

    def job_exec_wait(self, job):
        """seconds the GPU-side thread of that prepare waited for the host executor"""
        return float(self.lib.dvt_rv32_job_exec_wait_seconds(job))

    def prove_job(self, pk, job, want_bytes=True):
        """K0..K9 on a prepared, HBM-resident shard"""
        if not want_bytes:
            self.check(self.lib.dvt_rv32_prove_job(self.h, pk, job, None, None))
            return None
        out, n = u8p(), C.c_size_t()
        self.check(self.lib.dvt_rv32_prove_job(self.h, pk, job, C.byref(out), C.byref(n)))
        b = C.string_at(out, n.value)
        self.lib.dvt_free(C.cast(out, C.c_void_p))
        return b

    def check_job(self, pk, job, cap=256):
        """Trace rows of a prepared job against the AIR, on the GPU (dvt_rv32_check_job).  Returns (summary, findings):
        summary = dict(ok, violations, n_findings, bus_checked, unbalanced_buses, ms, error), findings = list of
        dict(shard, chip, log_n, violations, first_row, first_constraint), at most cap of them.  A job with violations or
        unbalanced buses is reported (ok False, error = the library's message), not raised; other failures raise."""
        arr = (CheckFinding * max(cap, 1))()
        s = CheckSummary()
        rc = self.lib.dvt_rv32_check_job(self.h, pk, job, arr, cap, C.byref(s))
        if rc not in (DVT_OK, DVT_ERR_REJECTED):
            self.check(rc)
        summary = dict(ok=rc == DVT_OK, violations=int(s.violations), n_findings=int(s.n_findings), bus_checked=int(s.bus_checked),
                       unbalanced_buses=int(s.unbalanced_buses), ms=float(s.ms), error=self.lib.dvt_last_error(self.h).decode() if rc else "")
        found = [dict(shard=int(f.shard), chip=int(f.chip), log_n=int(f.log_n), violations=int(f.r.violations), first_row=int(f.r.first_row),
                      first_constraint=int(f.r.first_constraint)) for f in arr[:min(int(s.n_findings), cap)]]
        return summary, found

    def job_profile(self, pk, job, log_edge_slots=0):
        """The execution report of a prepared job, tallied on the GPU from the cycle records of the shards it holds
        (dvt_rv32_job_profile): dict(summary, pc_count (numpy u64, one per instruction of the text), edges = [(from_pc, to_pc,
        count)] sorted, syscalls = {id: count}, opcodes = {mnemonic: count}).  log_edge_slots bounds the table of the indirect
        edges (0 = sized from the text); what it cannot hold is counted in summary["dropped_transfers"]."""
        rc, prof = _profile(lambda *out: self.lib.dvt_rv32_job_profile(self.h, pk, job, log_edge_slots, *out))
        self.check(rc)
        return prof

    def job_calltree(self, pk, job, log_arc_slots=0):
        """The call-tree report of a prepared job that holds every shard of its execution, from its cycle records on the GPU
        (dvt_rv32_job_calltree): dict(summary, arcs = [(caller_pc or None for the root, callee_pc, calls, cycles)] sorted,
        funcs = [(pc, calls, inclusive, self)] by self descending).  log_arc_slots bounds the table of the arcs (0 = sized
        from the text); what it cannot hold is counted in summary["dropped_frames"], and funcs is then empty."""
        rc, tree = _calltree(lambda *out: self.lib.dvt_rv32_job_calltree(self.h, pk, job, log_arc_slots, *out))
        self.check(rc)
        return tree

    def job_memory(self, pk, job):
        """The memory report of a prepared job, from the cycle records of the shards it holds on the GPU (dvt_rv32_job_memory):
        dict(summary, first_touch (numpy u64, one per instruction of the text), pages = [dict(page, words, first, loads,
        stores, pre_reads, pre_writes)] sorted by address).  Every figure is exact."""
        rc, mem = _memory(lambda *out: self.lib.dvt_rv32_job_memory(self.h, pk, job, *out))
        self.check(rc)
        return mem

    def job_watch(self, pk, job, queries, keep=16, summary=False):
        """Watchpoints on a prepared job, from the cycle records of the shards it holds on the GPU (dvt_rv32_job_watch): per query
        (watch_pc / watch_reg / watch_mem dicts, at most 16) dict(total = the exact number of hits, first = the first
        min(keep, total) hits in execution order, last = the last min(keep, total)); a hit is a dict of the fields of
        dvt_watch_hit.  keep <= 256.  summary=True: (that list, the summary dict)."""
        rc, found, s = _watch(lambda *io: self.lib.dvt_rv32_job_watch(self.h, pk, job, *io), list(queries), keep)
        self.check(rc)
        return (found, s) if summary else found

    def job_watch_times(self):
        """of the last job_watch: dict(count_ms, scan_ms, emit_ms (stream events, summed over members), emit_shards)"""
        out = (C.c_double * 4)()
        self.check(self.lib.dvt_rv32_job_watch_times(self.h, out))
        return dict(count_ms=out[0], scan_ms=out[1], emit_ms=out[2], emit_shards=int(out[3]))

    def job_snapshot(self, pk, job, at, ranges=(), frames=64):
        """The machine as it is before the record at `at` = (shard, row) of a prepared job executes (SNAP_EXIT: after the last
        record), from the cycle records the job holds on the GPU (dvt_rv32_job_snapshot): dict(summary, regs = 32 cells, words =
        the cells of `ranges` ((lo, hi) word addresses, snap_range() makes them; at most 16 ranges and 4096 words), frames =
        the innermost `frames` frames of the call stack).  A cell is a dict of the fields of dvt_snap_cell; its flags say
        where the value comes from, DVT_SNAP_NO_VALUE that the records do not hold it."""
        rc, snap = _snapshot(lambda *io: self.lib.dvt_rv32_job_snapshot(self.h, pk, job, *io), at, ranges, frames)
        self.check(rc)
        return snap

    def job_snapshot_times(self):
        """of the last job_snapshot: dict(reduce_ms, gather_ms, backtrace_ms), stream events summed over members"""
        out = (C.c_double * 3)()
        self.check(self.lib.dvt_rv32_job_snapshot_times(self.h, out))
        return dict(reduce_ms=out[0], gather_ms=out[1], backtrace_ms=out[2])

    def job_origin(self, pk, job, at, target, follow_addr=False, depth=DVT_ORIGIN_MAX_DEPTH, nodes=DVT_ORIGIN_MAX_NODES, edges=DVT_ORIGIN_MAX_EDGES):
        """Where the value of `target` (origin_reg() / origin_word()) before the record at `at` = (shard, row) of a prepared job
        comes from (SNAP_EXIT: after the last record): the backward data-flow slice over the cycle records the job holds on the
        GPU (dvt_rv32_job_origin), dict(summary, nodes, edges).  A node is one record (a dict of the fields of dvt_origin_node), in
        discovery order; edges[0] is the root, the input edges of node i are edges[first_edge : first_edge + n_edges]; an edge's
        `to` is its producer's node or DVT_ORIGIN_NONE with INITIAL / CUT in its flags.  follow_addr: also follow the address
        registers of loads and stores.  depth <= 64, nodes <= 1024, edges <= 8192."""
        rc, got = _origin(lambda *io: self.lib.dvt_rv32_job_origin(self.h, pk, job, *io), at, target, follow_addr, depth, nodes, edges)
        self.check(rc)
        return got

    def job_origin_times(self):
        """of the last job_origin: dict(reduce_ms, gather_ms (stream events summed over members, levels and passes), host_ms)"""
        out = (C.c_double * 3)()
        self.check(self.lib.dvt_rv32_job_origin_times(self.h, out))
        return dict(reduce_ms=out[0], gather_ms=out[1], host_ms=out[2])

    def job_uses(self, pk, job, at, target, follow_addr=False, depth=DVT_USES_MAX_DEPTH, fan=DVT_USES_DEFAULT_FAN, nodes=DVT_USES_MAX_NODES,
                 defs=DVT_USES_MAX_DEFS, edges=DVT_USES_MAX_EDGES):
        """Who reads the value `target` (uses_reg() / uses_word()) holds from the record at `at` = (shard, row) of a prepared job on,
        and what those readers produce: the forward data-flow slice over the cycle records the job holds on the GPU
        (dvt_rv32_job_uses; the rule: csrc/uses.h), dict(summary, nodes, defs, edges).  defs[0] is the root definition; a
        definition has its next writer (next_shard, next_row), the exact n_uses and its first min(fan, n_uses) uses
        edges[first_edge : first_edge + n_edges]; an edge's `to` is the consumer's node (or DVT_USES_NONE with CUT), whose own
        definitions are defs[first_def : first_def + n_defs].  depth <= 64, fan 1..16, nodes <= 1024, defs <= 4096, edges <= 8192."""
        rc, got = _uses(lambda *io: self.lib.dvt_rv32_job_uses(self.h, pk, job, *io), at, target, follow_addr, depth, fan, nodes, defs, edges)
        self.check(rc)
        return got

    def job_uses_times(self):
        """of the last job_uses: dict(next_ms, count_ms (count and scan), emit_ms, gather_ms (stream events summed over members,
        levels and passes), host_ms)"""
        out = (C.c_double * 5)()
        self.check(self.lib.dvt_rv32_job_uses_times(self.h, out))
        return dict(next_ms=out[0], count_ms=out[1], emit_ms=out[2], gather_ms=out[3], host_ms=out[4])

    def job_diverge(self, pk, job_a, job_b, start_a=DIVERGE_ENTRY, start_b=DIVERGE_ENTRY, max_pairs=0, rejoin=False, window=0, keep=16):
        """Where two prepared jobs of this handle (two executions of pk's guest; job_a may be job_b) part ways, from the cycle records
        both hold on the GPU (dvt_rv32_job_diverge; the rule: csrc/diverge.h): pair k is (A[start_a + k], B[start_b + k]).
        dict(summary, regs, first, last): summary has n_pairs (= the stop), reason (DVT_DIV_SPLIT .. _LIMIT), the data counts, the
        positions and records of pair `stop` (stop_a, stop_b) and of the deciding pair before it (prev_a, prev_b), with rejoin=True the
        rejoin positions; regs[r] says where register r was written with differing values and whether it is live at the stop;
        first / last are the first and last min(keep, n_data) data pairs.  keep <= 64, window <= 16384 (0: 4096)."""
        rc, got = _diverge(lambda *io: self.lib.dvt_rv32_job_diverge(self.h, pk, job_a, job_b, *io), start_a, start_b, max_pairs, rejoin, window, keep)
        self.check(rc)
        return got

    def job_diverge_times(self):
        """of the last job_diverge: dict(classify_ms, merge_ms, emit_ms (emit and gather), stream events summed over members and
        batches; host_ms)"""
        out = (C.c_double * 4)()
        self.check(self.lib.dvt_rv32_job_diverge_times(self.h, out))
        return dict(classify_ms=out[0], merge_ms=out[1], emit_ms=out[2], host_ms=out[3])

    def job_calltree_times(self):
        """milliseconds of the last job_calltree: dict(summary_ms, merge_ms, emit_ms)"""
        out = (C.c_double * 3)()
        self.check(self.lib.dvt_rv32_job_calltree_times(self.h, out))
        return dict(summary_ms=out[0], merge_ms=out[1], emit_ms=out[2])

    def bus_ledger(self, machine, log_buckets=20, cap_slots=1 << 16, seed=1):
        """a BusLedger on this handle: which tuples of the LogUp buses do not cancel over the tables it is given"""
        return BusLedger(self, machine, log_buckets, cap_slots, seed)

    def job_bus_tuples(self, pk, job, cap=4096):
        """The unmatched LogUp tuples of a prepared job (dvt_rv32_job_bus_tuples): (tuples, truncated); a tuple is a dict(bus,
        arity, net, n_send, n_recv, first_tag = shard position, first_chip, first_row, first_interaction, values)."""
        arr = (BusTuple * max(cap, 1))()
        n, trunc = C.c_size_t(), C.c_uint32()
        self.check(self.lib.dvt_rv32_job_bus_tuples(self.h, pk, job, arr, cap, C.byref(n), C.byref(trunc)))
        return _bus_tuples(arr, n.value), bool(trunc.value)

    def job_shard_chips(self, job, shard):
        """bit c set: shard `shard` (global position) has a table of chip c; 0 when the job does not hold the shard"""
        return int(self.lib.dvt_rv32_job_shard_chips(job, shard))

    def job_shard_chip_shape(self, job, shard, chip):
        """(main_w, log_n) of the main trace of chip `chip` of that shard (global position); DvtError(DVT_ERR_INPUT) when the job
        does not hold the shard or the shard has no table of the chip"""
        w, h = C.c_uint32(), C.c_uint32()
        rc = self.lib.dvt_rv32_job_shard_chip_shape(job, shard, chip, C.byref(w), C.byref(h))
        if rc:
            raise DvtError(rc, f"shard {shard} of this job has no table of chip {chip}")
        return int(w.value), int(h.value)

    def debug_device_traces(self, pk, job, shard=0):
        """K0 on the device for one shard, traces downloaded (canonical): (chips, pubs)"""
        blob, n = u32p(), C.c_size_t()
        self.check(self.lib.dvt_rv32_debug_device_traces(self.h, pk, job, shard, C.byref(blob), C.byref(n)))
        w = np.ctypeslib.as_array(blob, shape=(n.value,)).copy()
        self.lib.dvt_free(C.cast(blob, C.c_void_p))
        return _parse_blob(w)

    def debug_poke_cell(self, job, shard, chip, col, row, add):
        """Test hook (dvt_rv32_debug_poke_cell): adds the canonical field element `add` (1 .. p-1) to main-trace cell (col, row)
        of that chip's table of that shard (global position) of a prepared job.  Aux chips: in place, for the life of the
        job; byte / program: the base multiplicities every K0 starts from; cpu: the kept K0 output, until the shard's next K0
        (DvtError(DVT_ERR_UNSUPPORTED) when the shard holds no valid one).  The shard's phase 1 runs again before its next proof."""
        self.check(self.lib.dvt_rv32_debug_poke_cell(self.h, job, shard, chip, col, row, add))

    # ---- shard-level API (multi-GPU: ranks own shards; the headers are the only thing exchanged)
    def job_shards(self, job):
        return int(self.lib.dvt_rv32_job_shards(job))

    def job_shard_member(self, job, shard):
        """the device member that holds a shard (global position), -1 when the job does not hold it"""
        return int(self.lib.dvt_rv32_job_shard_member(job, shard))

    def job_shard_device_rows(self, job, shard):
        """bit c set: the rows of chip c of that shard (global position) were built on the GPU from events; 0 when the
        job does not hold the shard"""
        return int(self.lib.dvt_rv32_job_shard_device_rows(job, shard))

    def job_shard_kept(self, job, shard):
        """the DVT_KEEP_* tier of that shard (global position) from its last phase 1; -1 when the job does not hold the shard
        or no phase 1 of it has run"""
        return int(self.lib.dvt_rv32_job_shard_kept(job, shard))

    def job_shard_kept_bytes(self, job, shard):
        """the bytes that tier holds in HBM: the tree (TREE), tree + main LDEs + K0 buffers (FULL), 0 otherwise"""
        return int(self.lib.dvt_rv32_job_shard_kept_bytes(job, shard))

    def commit_shard(self, pk, job, shard):
        h = np.zeros(HEADER_WORDS, np.uint32)
        self.check(self.lib.dvt_rv32_commit_shard(self.h, pk, job, shard, h.ctypes.data_as(u32p)))
        return h

    def prove_shard(self, pk, job, shard, challenges, want_bytes=True):
        ch = np.ascontiguousarray(challenges, dtype=np.uint32)
        if not want_bytes:
            self.check(self.lib.dvt_rv32_prove_shard(self.h, pk, job, shard, ch.ctypes.data_as(u32p), None, None))
            return None
        out, n = u8p(), C.c_size_t()
        self.check(self.lib.dvt_rv32_prove_shard(self.h, pk, job, shard, ch.ctypes.data_as(u32p), C.byref(out), C.byref(n)))
        b = C.string_at(out, n.value)
        self.lib.dvt_free(C.cast(out, C.c_void_p))
        return b

    def assemble(self, job, shard_proofs):
        n = len(shard_proofs)
        arr = (C.c_char_p * n)(*shard_proofs)
        lens = (C.c_size_t * n)(*[len(x) for x in shard_proofs])
        out, m = u8p(), C.c_size_t()
        rc = self.lib.dvt_rv32_assemble(job, arr, lens, n, C.byref(out), C.byref(m))
        if rc:
            raise DvtError(rc, "dvt_rv32_assemble")
        b = C.string_at(out, m.value)
        self.lib.dvt_free(C.cast(out, C.c_void_p))
        return b

    def job_free(self, job):
        self.lib.dvt_job_free(self.h, job)

    def kernel_stats(self):
        """K1 / K2+K3 family totals of the last prove on a profile handle (HIP events on the prover stream)"""
        self.lib.dvt_last_kernel_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        out = (C.c_double * 9)()
        self.check(self.lib.dvt_last_kernel_stats(self.h, out))
        return dict(lde_ms=out[0], lde_alg_bytes=out[1], lde_calls=int(out[2]), merkle_ms=out[3], merkle_perms=out[4],
                    cells_main=out[5], cells_perm=out[6], cells_quotient=out[7], cells_prep=out[8])

    def stage_ms(self):
        out = (C.c_float * 6)()
        self.check(self.lib.dvt_last_stage_ms(self.h, out))
        return dict(zip(["commit_main", "permutation", "quotient", "openings", "fri", "total"], list(out)))
