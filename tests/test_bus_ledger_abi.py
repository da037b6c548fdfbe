"""The C ABI of the bus ledger (ABI version 8), without a GPU: symbols, the record's layout, NULL handles, and the host's
key function, which is the function the kernels key the rows with (csrc/ledger_key.h)."""
import ctypes as C
import os
import re

import numpy as np

from dvt_circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("dvt_stage_bus_ledger_new", "dvt_stage_bus_ledger_add", "dvt_stage_bus_ledger_add_tuple", "dvt_stage_bus_ledger_close",
           "dvt_stage_bus_ledger_collect", "dvt_stage_bus_ledger_result", "dvt_stage_bus_ledger_free", "dvt_rv32_job_bus_tuples")
u32p = C.POINTER(C.c_uint32)


def test_the_eight_symbols_are_exported_and_the_abi_is_8():
    lib = capi.load()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.dvt_abi_version() >= 8
    for name in ("bus_ledger", "job_bus_tuples"):
        assert hasattr(capi.Prover, name), name


def test_record_is_49_words_in_header_and_binding():
    assert C.sizeof(capi.BusTuple) == 4 * 49
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    assert int(re.search(r"#define DVT_LEDGER_MAX_ARITY (\d+)u", src).group(1)) == capi.LEDGER_MAX_ARITY == 40
    body = re.search(r"typedef struct \{([^}]*)\} dvt_bus_tuple;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.replace("uint32_t", "").split(",")]
    assert names == [f if f != "values" else "values[DVT_LEDGER_MAX_ARITY]" for f, _ in capi.BusTuple._fields_]


def test_every_call_refuses_a_null_handle():
    lib = capi.load()
    h, n32, n, t = C.c_void_p(), C.c_uint32(), C.c_size_t(), capi.BusTuple()
    v = (C.c_uint32 * 4)(1, 2, 3, 4)
    assert lib.dvt_stage_bus_ledger_new(None, b"toy", 10, 16, 1, C.byref(h)) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_bus_ledger_add(None, None, 0, None, None, 3, v, 0) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_bus_ledger_add_tuple(None, None, 1, v, 4, 1, 1, 0) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_bus_ledger_close(None, None, C.byref(n32)) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_bus_ledger_collect(None, None, 0, None, None, 3, v, 0) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_bus_ledger_result(None, None, C.byref(t), 1, C.byref(n), C.byref(n32)) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_bus_ledger_free(None, None) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_job_bus_tuples(None, None, None, C.byref(t), 1, C.byref(n), C.byref(n32)) == capi.DVT_ERR_INPUT


def key(seed, bus, values):
    v = np.ascontiguousarray(values, dtype=np.uint32)
    if v.size == 0:
        v = np.zeros(1, np.uint32)
    return int(capi.load().dvt_debug_ledger_key(seed, bus, len(values), v.ctypes.data_as(u32p)))


def test_key_is_deterministic_and_depends_on_every_input():
    rng = np.random.default_rng(8)
    vals = rng.integers(0, 2013265921, 40, dtype=np.uint32)
    base = key(7, 3, vals)
    assert base == key(7, 3, vals.copy())
    seen = {base, key(8, 3, vals), key(7, 4, vals)}
    assert len(seen) == 3
    for arity in range(40):            # the arity: a prefix is another tuple, also when the dropped values are zero
        seen.add(key(7, 3, vals[:arity]))
    assert len(seen) == 43
    assert key(7, 3, [0, 0]) != key(7, 3, [0]) != key(7, 3, [])
    for k in range(40):                # every value, by one unit and in its top bit
        for delta in (1, 1 << 30):
            w = vals.copy()
            w[k] ^= delta
            seen.add(key(7, 3, w))
    assert len(seen) == 43 + 80
    assert key(7, 3, [1, 2]) != key(7, 3, [2, 1])
