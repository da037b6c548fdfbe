"""The ABI of the trace-row checks without a GPU: the new symbols are exported, the ABI version moved, and the job check
refuses a NULL handle."""
import ctypes as C

from dvt_circuits_amd import capi


def test_check_symbols_are_exported():
    lib = capi.load()
    for name in ("dvt_stage_check_constraints", "dvt_stage_bus_sums", "dvt_rv32_check_job", "dvt_rv32_debug_poke_cell"):
        assert hasattr(lib, name), name


def test_abi_version_is_at_least_6():
    assert capi.load().dvt_abi_version() >= 6


def test_check_job_refuses_null_handle():
    lib = capi.load()
    s = capi.CheckSummary()
    assert lib.dvt_rv32_check_job(None, None, None, None, 0, C.byref(s)) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_check_job(None, None, None, None, 0, None) == capi.DVT_ERR_INPUT


def test_check_structs_match_the_header():
    """dvt_check_result 16 bytes, dvt_check_finding 12 + 4 (alignment) + 16, dvt_check_summary 8 + 3 * 4 + 4"""
    assert C.sizeof(capi.CheckResult) == 16 and C.sizeof(capi.CheckFinding) == 32 and C.sizeof(capi.CheckSummary) == 24
