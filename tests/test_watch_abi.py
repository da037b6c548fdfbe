"""The watchpoint entry points of the C ABI (no GPU): they exist, the structs have the sizes of include/dvt_prover.h, and every
input error of the issue is refused with DVT_ERR_INPUT and a text."""
import ctypes as C

import pytest

from dvt_circuits_amd import capi
from tests import guests

ELF = guests.arith()[0]


def test_entry_points_sizes_and_version():
    lib = capi.load()
    assert lib.dvt_abi_version() >= 16
    for name in ("dvt_rv32_job_watch", "dvt_rv32_job_watch_times", "dvt_execute_watch"):
        assert hasattr(lib, name), name
    assert (C.sizeof(capi.WatchQuery), C.sizeof(capi.WatchHit), C.sizeof(capi.WatchSummary)) == (40, 64, 40)
    assert (capi.DVT_WATCH_MAX_QUERIES, capi.DVT_WATCH_MAX_KEEP, capi.DVT_WATCH_SPAN) == (16, 256, 4096)
    assert (capi.DVT_WATCH_PC, capi.DVT_WATCH_REG, capi.DVT_WATCH_MEM) == (1, 2, 3)
    flags = (capi.DVT_WATCH_LOAD, capi.DVT_WATCH_STORE, capi.DVT_WATCH_PRE_READ, capi.DVT_WATCH_PRE_WRITE, capi.DVT_WATCH_VALUE, capi.DVT_WATCH_HIT_NO_VALUE)
    assert flags == (1, 2, 4, 8, 16, 32)
    # the header says the same
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvt_prover.h")).read()
    for line in ("#define DVT_WATCH_MAX_QUERIES 16", "#define DVT_WATCH_MAX_KEEP 256", "#define DVT_WATCH_SPAN 4096",
                 "enum { DVT_WATCH_PC = 1, DVT_WATCH_REG = 2, DVT_WATCH_MEM = 3 };"):
        assert line in text, line


def test_constructors():
    q = capi.watch_pc(0x200010)
    assert (q["kind"], q["lo"], q["hi"], q["flags"]) == (capi.DVT_WATCH_PC, 0x200010, 0x200014, 0)
    assert (q["from_shard"], q["from_row"], q["to_shard"], q["to_row"]) == (0, 0, 0xFFFFFFFF, 0xFFFFFFFF)
    q = capi.watch_reg(2, value=0x7FF0, mask=0xFFF0, window=((3, 100), (5, 0)))
    assert (q["kind"], q["lo"], q["flags"], q["want"], q["mask"]) == (capi.DVT_WATCH_REG, 2, capi.DVT_WATCH_VALUE, 0x7FF0, 0xFFF0)
    assert (q["from_shard"], q["from_row"], q["to_shard"], q["to_row"]) == (3, 100, 5, 0)
    q = capi.watch_mem(0x400000, 0x400040, flags=capi.DVT_WATCH_STORE)
    assert (q["kind"], q["lo"], q["hi"], q["flags"]) == (capi.DVT_WATCH_MEM, 0x400000, 0x400040, capi.DVT_WATCH_STORE)


def bad_queries():
    ok = capi.watch_pc(0x200000)
    return {
        "no queries": ([], 4),
        "17 queries": ([ok] * 17, 4),
        "cap_each 257": ([ok], 257),
        "unknown kind 0": ([dict(ok, kind=0)], 4),
        "unknown kind 4": ([dict(ok, kind=4)], 4),
        "unknown flag": ([dict(capi.watch_mem(0x400000), flags=capi.DVT_WATCH_LOAD | 64)], 4),
        "the hit's flag in a query": ([dict(capi.watch_mem(0x400000), flags=capi.DVT_WATCH_LOAD | capi.DVT_WATCH_HIT_NO_VALUE)], 4),
        "a direction on a pc query": ([dict(ok, flags=capi.DVT_WATCH_LOAD)], 4),
        "a direction on a register query": ([dict(capi.watch_reg(2), flags=capi.DVT_WATCH_STORE)], 4),
        "memory query without a direction": ([dict(capi.watch_mem(0x400000), flags=0)], 4),
        "pc lo == hi": ([capi.watch_pc(0x200000, 0x200000)], 4),
        "memory lo > hi": ([capi.watch_mem(0x400010, 0x400000)], 4),
        "register 0": ([dict(capi.watch_reg(1), lo=0)], 4),
        "register 32": ([dict(capi.watch_reg(1), lo=32)], 4),
        "from == to": ([capi.watch_pc(0x200000, window=((2, 5), (2, 5)))], 4),
        "from > to": ([capi.watch_pc(0x200000, window=((2, 5), (1, 900)))], 4),
        "the second query is bad": ([ok, dict(ok, kind=9)], 4),
    }


@pytest.mark.parametrize("what", sorted(bad_queries()))
def test_input_errors_are_refused(what):
    queries, keep = bad_queries()[what]
    rc, rep, found, err = capi.execute_watch(ELF, [], queries, keep=keep)
    assert rc == capi.DVT_ERR_INPUT and found is None and err, (what, rc, err)
    assert rep["cycles"] == 0    # (refused before the guest runs)


def test_null_arrays_are_refused():
    lib = capi.load()
    q = (capi.WatchQuery * 1)(capi.WatchQuery(**capi.watch_pc(0, 0xFFFFFFFF)))
    hits, totals, s = (capi.WatchHit * 8)(), (C.c_uint64 * 1)(), capi.WatchSummary()
    rep, err = capi.Report(), C.c_char_p()

    def call(q, n, keep, hits, totals, s):
        return lib.dvt_execute_watch(ELF, len(ELF), None, 0, 0, 0, q, n, keep, hits, totals, s, C.byref(rep), C.byref(err))
    assert call(q, 1, 4, hits, totals, C.byref(s)) == capi.DVT_OK and totals[0] >= 1
    assert call(None, 1, 4, hits, totals, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(q, 1, 4, None, totals, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(q, 1, 4, hits, None, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(q, 1, 4, hits, totals, None) == capi.DVT_ERR_INPUT
    # totals alone: cap_each 0 needs no hit array
    assert call(q, 1, 0, None, totals, C.byref(s)) == capi.DVT_OK and totals[0] >= 1 and s.cap_each == 0
    # a shard size outside 4..22
    assert lib.dvt_execute_watch(ELF, len(ELF), None, 0, 0, 23, q, 1, 4, hits, totals, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT


def test_the_summary_of_a_call():
    q = (capi.WatchQuery * 1)(capi.WatchQuery(**capi.watch_pc(0, 0xFFFFFFFF)))
    hits, totals, s = (capi.WatchHit * 2)(), (C.c_uint64 * 1)(), capi.WatchSummary()
    rep, err = capi.Report(), C.c_char_p()
    rc = capi.load().dvt_execute_watch(ELF, len(ELF), None, 0, 0, 10, q, 1, 1, hits, totals, C.byref(s), C.byref(rep), C.byref(err))
    assert rc == capi.DVT_OK and totals[0] == s.cycles == rep.cycles and s.shards_searched == s.shards_total == (rep.cycles + 1023) // 1024
    assert (s.n_queries, s.cap_each, s.span) == (1, 1, capi.DVT_WATCH_SPAN)
    assert (hits[0].shard, hits[0].row) == (1, 0) and (hits[1].shard, hits[1].row) == (s.shards_total, (rep.cycles - 1) % 1024)
