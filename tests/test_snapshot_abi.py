"""The snapshot entry points of the C ABI (no GPU): they exist, the structs have the sizes of include/dvt_prover.h, every input
error of the issue is refused with DVT_ERR_INPUT and a text, and the size limits are the ones stated."""
import ctypes as C
import os

import pytest

from dvt_circuits_amd import capi
from tests import guests

ELF = guests.arith()[0]
ADDR_LIMIT = 0x38000000
BASE = 0x400000


def test_entry_points_sizes_and_version():
    lib = capi.load()
    assert lib.dvt_abi_version() >= 17
    for name in ("dvt_rv32_job_snapshot", "dvt_rv32_job_snapshot_times", "dvt_execute_snapshot"):
        assert hasattr(lib, name), name
    assert (C.sizeof(capi.SnapRange), C.sizeof(capi.SnapCell), C.sizeof(capi.SnapFrame), C.sizeof(capi.SnapSummary)) == (8, 24, 24, 80)
    assert (capi.DVT_SNAP_MAX_RANGES, capi.DVT_SNAP_MAX_WORDS, capi.DVT_SNAP_SPAN) == (16, 4096, 4096)
    flags = (capi.DVT_SNAP_INITIAL, capi.DVT_SNAP_FROM_BEFORE, capi.DVT_SNAP_FROM_AFTER, capi.DVT_SNAP_LOAD, capi.DVT_SNAP_STORE, capi.DVT_SNAP_IMAGE,
             capi.DVT_SNAP_NO_VALUE, capi.DVT_SNAP_UNTOUCHED)
    assert flags == (1, 2, 4, 8, 16, 32, 64, 128)
    # the header says the same
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvt_prover.h")).read()
    for line in ("#define DVT_SNAP_MAX_RANGES 16", "#define DVT_SNAP_MAX_WORDS 4096", "#define DVT_SNAP_SPAN 4096",
                 "enum { DVT_SNAP_INITIAL = 1, DVT_SNAP_FROM_BEFORE = 2, DVT_SNAP_FROM_AFTER = 4, DVT_SNAP_LOAD = 8, DVT_SNAP_STORE = 16, DVT_SNAP_IMAGE = 32,",
                 "DVT_SNAP_NO_VALUE = 64, DVT_SNAP_UNTOUCHED = 128 };"):
        assert line in text, line


def test_snap_range_covers_the_bytes():
    assert capi.snap_range(0x400000, 4) == (0x400000, 0x400004)
    assert capi.snap_range(0x400002, 4) == (0x400000, 0x400008)
    assert capi.snap_range(0x400003, 1) == (0x400000, 0x400004)
    assert capi.snap_range(0x400004, 64) == (0x400004, 0x400044)
    assert capi.snap_range(0x400000) == (0x400000, 0x400004)


def bad_ranges():
    one = (BASE, BASE + 4)
    return {
        "17 ranges": [(BASE + 8 * k, BASE + 8 * k + 4) for k in range(17)],
        "4097 words in one range": [(BASE, BASE + 4 * 4097)],
        "4097 words in two ranges": [(BASE, BASE + 4 * 4096), one],
        "lo not aligned": [(BASE + 2, BASE + 8)],
        "hi not aligned": [(BASE, BASE + 7)],
        "an empty range": [(BASE, BASE)],
        "lo above hi": [(BASE + 8, BASE)],
        "a range at the address limit": [(ADDR_LIMIT, ADDR_LIMIT + 4)],
        "a range across the address limit": [(ADDR_LIMIT - 4, ADDR_LIMIT + 4)],
        "a range above the address limit": [(0xFFFFFF00, 0xFFFFFF10)],
        "the second range is bad": [one, (BASE + 1, BASE + 5)],
    }


@pytest.mark.parametrize("what", sorted(bad_ranges()))
def test_input_errors_are_refused(what):
    rc, rep, snap, err = capi.execute_snapshot(ELF, [], capi.SNAP_EXIT, bad_ranges()[what])
    assert rc == capi.DVT_ERR_INPUT and snap is None and err, (what, rc, err)
    assert rep["cycles"] == 0    # (refused before the guest runs)


def test_the_size_limits_are_reached():
    """16 ranges and 4096 words are taken; the last word below the address limit is a word like any other"""
    rc, rep, snap, err = capi.execute_snapshot(ELF, [], capi.SNAP_EXIT, [(BASE + 1024 * k, BASE + 1024 * k + 1024) for k in range(16)])
    assert rc == capi.DVT_OK and snap["summary"]["n_words"] == len(snap["words"]) == 4096, err
    assert [c["addr"] for c in snap["words"][:257:256]] == [BASE, BASE + 1024]
    rc, rep, snap, err = capi.execute_snapshot(ELF, [], capi.SNAP_EXIT, [(ADDR_LIMIT - 4, ADDR_LIMIT)])
    assert rc == capi.DVT_OK and snap["words"][0]["addr"] == ADDR_LIMIT - 4, err
    assert snap["words"][0]["flags"] == capi.DVT_SNAP_NO_VALUE | capi.DVT_SNAP_UNTOUCHED


def test_null_arrays_and_small_capacities_are_refused():
    lib = capi.load()
    rs = (capi.SnapRange * 2)(capi.SnapRange(BASE, BASE + 16), capi.SnapRange(BASE + 64, BASE + 80))
    regs, words, frames, s = (capi.SnapCell * 32)(), (capi.SnapCell * 8)(), (capi.SnapFrame * 4)(), capi.SnapSummary()
    rep, err = capi.Report(), C.c_char_p()

    def call(rs, n, regs, words, cap_words, frames, cap_frames, s, log_shard=0):
        return lib.dvt_execute_snapshot(ELF, len(ELF), None, 0, 0, log_shard, 0xFFFFFFFF, 0xFFFFFFFF, rs, n, regs, words, cap_words, frames, cap_frames, s,
                                        C.byref(rep), C.byref(err))
    assert call(rs, 2, regs, words, 8, frames, 4, C.byref(s)) == capi.DVT_OK and s.n_words == 8 and s.cycles == rep.cycles
    assert call(None, 2, regs, words, 8, frames, 4, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(rs, 2, None, words, 8, frames, 4, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(rs, 2, regs, None, 8, frames, 4, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(rs, 2, regs, words, 8, None, 4, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(rs, 2, regs, words, 8, frames, 4, None) == capi.DVT_ERR_INPUT
    assert call(rs, 2, regs, words, 7, frames, 4, C.byref(s)) == capi.DVT_ERR_INPUT    # cap_words below the words asked for
    # no ranges need no word array, no frames no frame array
    assert call(None, 0, regs, None, 0, None, 0, C.byref(s)) == capi.DVT_OK and s.n_words == 0 and s.n_frames == 0 and s.depth >= 1
    # a shard size outside 4..22
    assert call(rs, 2, regs, words, 8, frames, 4, C.byref(s), log_shard=23) == capi.DVT_ERR_INPUT


def test_the_summary_of_a_call():
    rc, rep, snap, err = capi.execute_snapshot(ELF, [], (2, 5), [(BASE, BASE + 8)], log_shard=10)
    s = snap["summary"]
    assert rc == capi.DVT_OK and s["cycles"] == rep["cycles"] and s["shards_total"] == (rep["cycles"] + 1023) // 1024, err
    assert (s["position"], s["shard"], s["row"], s["span"], s["n_words"]) == (1024 + 5, 2, 5, capi.DVT_SNAP_SPAN, 2)
    assert snap["regs"][0] == dict(addr=0, value=0, flags=0, shard=0, row=0, pc=0)
    # a position past the end is the end, whatever its spelling
    end = capi.execute_snapshot(ELF, [], capi.SNAP_EXIT, [(BASE, BASE + 8)], log_shard=10)[2]
    far = capi.execute_snapshot(ELF, [], (s["shards_total"] + 3, 0), [(BASE, BASE + 8)], log_shard=10)[2]
    for part in ("regs", "words", "frames"):
        assert end[part] == far[part]
    assert end["summary"]["position"] == far["summary"]["position"] == rep["cycles"]
    assert (end["summary"]["shard"], end["summary"]["row"]) == (s["shards_total"], rep["cycles"] - 1024 * (s["shards_total"] - 1))
