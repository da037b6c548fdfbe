"""The ABI of the forgery hunt without a GPU: the three symbols are exported, the ABI version moved to 9, the record has the
header's 36 bytes, and every entry refuses a NULL handle."""
import ctypes as C

from dvt_circuits_amd import capi


def test_hunt_symbols_are_exported():
    lib = capi.load()
    for name in ("dvt_stage_hunt_cells", "dvt_stage_hunt_pairs", "dvt_rv32_hunt_shard", "dvt_rv32_job_shard_chip_shape"):
        assert hasattr(lib, name), name


def test_abi_version_is_at_least_9():
    assert capi.load().dvt_abi_version() >= 9


def test_escape_matches_the_header():
    assert C.sizeof(capi.Escape) == 36 and capi.HUNT_MAX_DELTAS == 8


def test_hunts_refuse_a_null_handle():
    lib = capi.load()
    d = (C.c_uint32 * 1)(1)
    counts = (C.c_uint32 * 4)()
    n, t = C.c_uint64(), C.c_uint64()
    assert lib.dvt_stage_hunt_cells(None, b"toy", 1, None, None, 3, None, 1, d, 1, 0, 8, 0, counts, None) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_hunt_pairs(None, b"toy", 1, None, None, 3, None, 1, d, 1, None, 0, 0, 0, 8, 0, None, 0, C.byref(n), C.byref(t)) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_hunt_shard(None, None, None, 0, 0, 1, d, 1, 0, None, 0, 0, 0, 8, 0, counts, None, None, 0, None, None) == capi.DVT_ERR_INPUT
    w, h = C.c_uint32(), C.c_uint32()
    assert lib.dvt_rv32_job_shard_chip_shape(None, 0, 0, C.byref(w), C.byref(h)) == capi.DVT_ERR_INPUT
