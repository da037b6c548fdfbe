"""The C ABI of the join hunt (ABI version 10) without a GPU: the six symbols and the binding, the two records' layouts in header
and binding, NULL handles and NULL arguments, and what a machine without a HIP device answers.  The argument checks that
need a handle (a supply table after a window, overlapping windows, a tag >= 2^16, ...) need a device to make one: they are
in tests/test_gpu_hunt_join.py."""
import ctypes as C
import os
import re

from dvt_circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvt_stage_hunt_join_new", "dvt_stage_hunt_join_supply", "dvt_stage_hunt_join_add", "dvt_stage_hunt_join_match",
           "dvt_stage_hunt_join_result", "dvt_stage_hunt_join_free", "dvt_rv32_hunt_join_job")


def test_symbols_are_exported_and_the_abi_is_10():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.dvt_abi_version() >= 10
    assert hasattr(capi.Prover, "hunt_join") and hasattr(capi.Prover, "hunt_join_job")


def _fields(src, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n.strip() for decl in body.split(";") if decl.strip() for n in re.sub(r"uint(32|64)_t", "", decl).split(",")]


def test_records_match_the_header():
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    assert C.sizeof(capi.JoinCell) == 28 and C.sizeof(capi.JoinSummary) == 72 and C.sizeof(capi.JoinWindow) == 16
    assert _fields(src, "dvt_join_window") == [f for f, _ in capi.JoinWindow._fields_]
    assert _fields(src, "dvt_join_cell") == [f for f, _ in capi.JoinCell._fields_]
    assert _fields(src, "dvt_join_summary") == [f for f, _ in capi.JoinSummary._fields_]
    for name, value in (("RECORDS", capi.JOIN_TRUNC_RECORDS), ("ABSORBED", capi.JOIN_TRUNC_ABSORBED), ("PROBES", capi.JOIN_TRUNC_PROBES),
                        ("OUTPUT", capi.JOIN_TRUNC_OUTPUT)):
        assert int(re.search(r"#define DVT_JOIN_TRUNC_%s (\d+)u" % name, src).group(1)) == value
    assert int(re.search(r"#define DVT_JOIN_NO_GROUP (0x[0-9a-f]+)u", src).group(1), 16) == capi.JOIN_NO_GROUP


def test_every_call_refuses_a_null_handle():
    lib = capi.load()
    h, n, m = C.c_void_p(), C.c_size_t(), C.c_size_t()
    d = (C.c_uint32 * 1)(1)
    cell, sm = capi.JoinCell(), capi.JoinSummary()
    assert lib.dvt_stage_hunt_join_new(None, b"toy", 1, d, 1, 0, 0, 0, C.byref(h)) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_hunt_join_supply(None, None, 0, None, None, 8, None) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_hunt_join_add(None, None, 0, 2, None, None, 4, None, 0, 16, None, 0, 0) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_hunt_join_match(None, None, C.byref(sm)) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_hunt_join_result(None, None, C.byref(cell), 1, C.byref(n), C.byref(cell), 1, C.byref(m)) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_hunt_join_free(None, None) == capi.DVT_ERR_INPUT
    w = capi.JoinWindow(0, 2, 0, 16)
    assert lib.dvt_rv32_hunt_join_job(None, None, None, C.byref(w), 1, None, 0, 1, d, 1, None, None, 0, 0, 0, 0, C.byref(sm), C.byref(cell), 1,
                                      C.byref(n), C.byref(cell), 1, C.byref(m)) == capi.DVT_ERR_INPUT


def test_without_a_device_no_handle_is_made_and_with_one_the_checks_answer_before_any_launch():
    """DVT_ERR_DEVICE where there is no HIP device; where there is one, the DVT_ERR_INPUT cases of `new` and the NULL join"""
    lib = capi.load()
    try:
        p = capi.Prover()
    except capi.DvtError as e:
        assert e.code == capi.DVT_ERR_DEVICE
        return
    try:
        h = C.c_void_p()
        P = 2013265921
        for deltas, kw in (([], {}), ([0], {}), ([P], {}), (list(range(1, 10)), {}), ([1], dict(cap=(1 << 22) + 1)), ([1], dict(slots=5)),
                           ([1], dict(slots=27)), ([1], dict(machine=b"nope"))):
            d = (C.c_uint32 * max(len(deltas), 1))(*deltas)
            rc = lib.dvt_stage_hunt_join_new(p.h, kw.get("machine", b"toy"), 1, d, len(deltas), kw.get("cap", 16), 16, kw.get("slots", 0), C.byref(h))
            assert rc == capi.DVT_ERR_INPUT and not h.value, (deltas, kw)
        sm = capi.JoinSummary()
        assert lib.dvt_stage_hunt_join_match(p.h, None, C.byref(sm)) == capi.DVT_ERR_INPUT
        assert lib.dvt_stage_hunt_join_free(p.h, None) == capi.DVT_ERR_INPUT
    finally:
        p.close()
