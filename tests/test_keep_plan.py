"""The admission rule of "keep_phase1" (csrc/keep_plan.h through dvt_debug_keep_plan): what a committed shard keeps in HBM for
phase 2.  Host only: the rule takes byte counts and no device state.  The walk over long jobs is a condition on the rule,
checked with the model of the pipeline that DESIGN.md section 8 states; it is not a measurement."""
import ctypes as C

import pytest

from dvt_circuits_amd import capi

NONE, TREE, FULL = capi.DVT_KEEP_NONE, capi.DVT_KEEP_TREE, capi.DVT_KEEP_FULL
GB = 10 ** 9
TOTAL, RESERVE = 288 * GB, 24 * GB
F, T, UP = 2950 * 10 ** 6, 268 * 10 ** 6, 100 * 10 ** 6   # a 2^21-cycle shard: kept in full, its tree, what its upload allocates
L = T + UP


def restated(mode, free, total, reserve, full, tree, later, remaining, known, cap, kept):
    """the rule as the issue states it"""
    if mode == 0:
        return NONE
    if mode == 1:
        return FULL if free > reserve else NONE
    if free > reserve + (full - tree) + remaining * later and (known or free > total * 3 // 4) and (cap < 0 or kept < cap):
        return FULL
    return TREE if free > reserve else NONE


def test_constants_mirror_the_header():
    assert (NONE, TREE, FULL) == (0, 1, 2)


@pytest.mark.parametrize("free", [0, 1, RESERVE - 1, RESERVE, RESERVE + 1, RESERVE + F, TOTAL, 2 ** 64 - 1])
def test_modes_0_and_1(free):
    for reserve in (0, 1, RESERVE, TOTAL):
        for remaining, known, cap, kept in ((0, True, -1, 0), (500, False, 0, 7), (3, True, 2, 2)):
            assert capi.keep_plan(0, free, TOTAL, reserve, F, T, L, remaining, known, cap, kept) == NONE
            want = FULL if free > reserve else NONE   # (free == reserve is not FULL; R, the count and the cap are not read)
            assert capi.keep_plan(1, free, TOTAL, reserve, F, T, L, remaining, known, cap, kept) == want


@pytest.mark.parametrize("remaining", [0, 1, 7, 510])
def test_mode_2_full_boundary(remaining):
    edge = RESERVE + (F - T) + remaining * L
    assert capi.keep_plan(2, edge, TOTAL, RESERVE, F, T, L, remaining, True) == TREE
    assert capi.keep_plan(2, edge + 1, TOTAL, RESERVE, F, T, L, remaining, True) == FULL
    assert capi.keep_plan(2, edge - 1, TOTAL, RESERVE, F, T, L, remaining, True) == TREE


def test_mode_2_reserve_boundary():
    assert capi.keep_plan(2, RESERVE, TOTAL, RESERVE, F, T, L, 0, True) == NONE
    assert capi.keep_plan(2, RESERVE - 1, TOTAL, RESERVE, F, T, L, 0, True) == NONE
    assert capi.keep_plan(2, RESERVE + 1, TOTAL, RESERVE, F, T, L, 0, True) == TREE
    assert capi.keep_plan(2, RESERVE + (F - T) + 1, TOTAL, RESERVE, F, T, L, 0, True) == FULL


@pytest.mark.parametrize("total", [TOTAL, TOTAL + 1, TOTAL + 2, TOTAL + 3])
def test_mode_2_unknown_count_takes_the_first_quarter_only(total):
    edge = total * 3 // 4
    assert edge > RESERVE + (F - T) + 2 * L
    assert capi.keep_plan(2, edge, total, RESERVE, F, T, L, 2, False) == TREE
    assert capi.keep_plan(2, edge, total, RESERVE, F, T, L, 2, True) == FULL
    assert capi.keep_plan(2, edge + 1, total, RESERVE, F, T, L, 2, False) == FULL


def test_mode_2_cap():
    free = 200 * GB
    assert capi.keep_plan(2, free, TOTAL, RESERVE, F, T, L, 0, True, 0, 0) == TREE
    assert capi.keep_plan(2, free, TOTAL, RESERVE, F, T, L, 0, True, 3, 2) == FULL
    assert capi.keep_plan(2, free, TOTAL, RESERVE, F, T, L, 0, True, 3, 3) == TREE
    assert capi.keep_plan(2, free, TOTAL, RESERVE, F, T, L, 0, True, 3, 4) == TREE
    for kept in (0, 1, 10 ** 6, 2 ** 63):   # -1 never binds
        assert capi.keep_plan(2, free, TOTAL, RESERVE, F, T, L, 0, True, -1, kept) == FULL
    assert capi.keep_plan(2, RESERVE, TOTAL, RESERVE, F, T, L, 0, True, 0, 0) == NONE   # (the cap turns FULL into TREE, nothing else)


def test_mode_2_sums_beyond_64_bits_do_not_fit():
    big = 2 ** 64 - 1
    assert capi.keep_plan(2, big, big, RESERVE, F, T, big, 2, True) == TREE
    assert capi.keep_plan(2, big, big, big - 1, F, T, L, 0, True) == TREE
    assert capi.keep_plan(2, big, big, RESERVE, T, F, L, 0, True) == FULL   # (a tree larger than the whole: nothing extra to fit)


def test_every_other_mode_value_reads_as_1():
    for mode in (-1, 3, 100):
        assert capi.keep_plan(mode, RESERVE + 1, TOTAL, RESERVE, F, T, L, 500, False, 0, 0) == FULL
        assert capi.keep_plan(mode, RESERVE, TOTAL, RESERVE, F, T, L, 0, True, -1, 0) == NONE


def _walk(shards):
    """The model of one prepare on one device: 280 of 288 GB free at the start; shard i is uploaded, then admitted, when the
    fast pass has found min(S, 4 i + 9) shards.  Returns the count per tier."""
    free, count = 280 * GB, [0, 0, 0]
    for i in range(shards):
        free -= UP
        found = min(shards, 4 * i + 9)
        args = (2, free, TOTAL, RESERVE, F, T, L, found - i - 1, found == shards, -1, count[FULL])
        tier = capi.keep_plan(*args)
        assert tier == restated(*args), "shard %d of %d: %r" % (i, shards, args)
        count[tier] += 1
        free -= (0, T, F)[tier]
        assert free > 0
    return count


@pytest.mark.parametrize("shards,full,tree", [(32, 32, 0), (90, 83, 7), (128, 77, 51), (256, 60, 196), (384, 42, 342), (511, 25, 486)])
def test_walk_over_long_jobs(shards, full, tree):
    """no shard keeps nothing up to the 511 shards of the reference's finalization execution, and a job that fits keeps
    every shard in full"""
    assert _walk(shards) == [0, tree, full]


def test_abi_surface():
    lib = capi.load()
    assert lib.dvt_abi_version() >= 13
    for name in ("dvt_rv32_job_shard_kept", "dvt_rv32_job_shard_kept_bytes", "dvt_debug_keep_plan"):
        assert getattr(lib, name)
    assert lib.dvt_rv32_job_shard_kept(None, 0) == -1
    assert lib.dvt_rv32_job_shard_kept_bytes(None, 0) == 0
    assert lib.dvt_rv32_job_shard_kept_bytes.restype is C.c_uint64
