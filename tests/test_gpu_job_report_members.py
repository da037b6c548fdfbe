"""GPU tests of the per-member passes of the five record reports (csrc/capi_report.hip: dvt_rv32_job_profile, _calltree, _memory,
_watch and _snapshot) on handles whose members do not hold equal shares: a member that holds no shard at all (a one-shard job
on two members) and members that hold 3, 2 and 2 shards (seven shards on three members).

Each case prepares the same guest on a one-device handle and on the multi-member handle, runs all five reports on both and
asserts that they are equal once the wall-clock "ms" fields are removed, and equal to the host path's (dvt_execute_*; the
host's profile, call tree and memory report run at the default shard size, so their shard counts are left out as well).
Every comparison is of exact integers and whole lists."""
import functools
import math

import pytest

from tests._snapshot_ref import EXIT
from tests.test_watch_host import run_of, standard_queries, watched

pytestmark = pytest.mark.gpu
Q, POW, LOG_SHARD, KEEP = 6, 5, 14, 5
SHARD_COUNTS = ("shards_total", "shards_tallied")


def _plain(x, drop=("ms",)):
    """the report without the keys of `drop`, arrays as lists"""
    if isinstance(x, dict):
        return {k: _plain(v, drop) for k, v in x.items() if k not in drop}
    if isinstance(x, (list, tuple)):
        return [_plain(v, drop) for v in x]
    return x.tolist() if hasattr(x, "tolist") else x


def _sp_range(run):
    """32 words around the stack pointer the guest ends with, inside guest memory"""
    lo = min(max((run.reg[2] & ~3) - 64, 0), 0x38000000 - 128)
    return [(lo, lo + 128)]


@functools.lru_cache(maxsize=None)
def _device(name, extra, places):
    """(the five reports of the guest's job on a handle with `extra` in its config, the times after them, the job's shards)"""
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    elf, stdin = watched(name)
    run = run_of(name, LOG_SHARD)
    queries, ranges = standard_queries(run), _sp_range(run)
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, LOG_SHARD, extra))
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin))
    try:
        n = p.job_shards(job)
        found, summary = p.job_watch(pk, job, queries, keep=KEEP, summary=True)
        got = dict(profile=p.job_profile(pk, job), calltree=p.job_calltree(pk, job), memory=p.job_memory(pk, job), watch=found,
                   watch_summary=summary, snapshots=[p.job_snapshot(pk, job, at, ranges) for at in places])
        times = dict(calltree=p.job_calltree_times(), watch=p.job_watch_times(), snapshot=p.job_snapshot_times())
        none = p.job_watch(pk, job, queries, keep=0)
        assert [f["total"] for f in none] == [f["total"] for f in found]
        times["watch_keep_0"] = p.job_watch_times()
    finally:
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    return got, times, n


@functools.lru_cache(maxsize=None)
def _host(name, places):
    from dvt_circuits_amd import capi

    elf, stdin = watched(name)
    run = run_of(name, LOG_SHARD)
    queries, ranges = standard_queries(run), _sp_range(run)
    got = {}
    for key, call in (("profile", capi.execute_profile), ("calltree", capi.execute_calltree), ("memory", capi.execute_memory)):
        rc, rep, got[key], err = call(elf, list(stdin))
        assert rc == 0, err
    rc, rep, got["watch"], err = capi.execute_watch(elf, list(stdin), queries, keep=KEEP, log_shard=LOG_SHARD)
    assert rc == 0, err
    got["snapshots"] = []
    for at in places:
        rc, rep, snap, err = capi.execute_snapshot(elf, list(stdin), at, ranges, log_shard=LOG_SHARD)
        assert rc == 0, err
        got["snapshots"].append(snap)
    return got


def _check(name, extra, places, shards, shares):
    one, _, n_one = _device(name, "", places)
    many, _, n_many = _device(name, extra, places)
    assert n_one == n_many == shards == len(run_of(name, LOG_SHARD).shards)
    assert many["profile"]["summary"]["shards_tallied"] == sum(shares) == shards      # (members hold `shares` shards each)
    assert _plain(many) == _plain(one)
    host = _host(name, places)
    for key in ("profile", "calltree", "memory"):
        assert _plain(many[key], ("ms",) + SHARD_COUNTS) == _plain(host[key], ("ms",) + SHARD_COUNTS), key
    for key in ("watch", "snapshots"):
        assert _plain(many[key]) == _plain(host[key]), key
    for at, snap in zip(places, many["snapshots"]):
        assert len(snap["words"]) == 32 and snap["summary"]["n_words"] == 32, at


IDLE = ("arith", ', "devices": [0, 0]')


def _idle_places():
    cycles = run_of(IDLE[0], LOG_SHARD).cycles
    assert 2 < cycles <= 1 << LOG_SHARD
    return ((1, 0), (1, cycles // 2), EXIT)


def test_a_member_that_holds_no_shard():
    """one shard on two members: member 1 is idle in every pass of every report"""
    _check(*IDLE, _idle_places(), 1, (1, 0))


def test_members_with_unequal_shares():
    """seven shards on three members: 3, 2 and 2; the snapshot's position lies in shard 4, which member 0 holds"""
    _check("bignum", ', "devices": [0, 0, 0]', ((4, 5000),), 7, (3, 2, 2))


def test_the_times_after_a_call_with_an_idle_member():
    _, times, n = _device(*IDLE, _idle_places())
    assert n == 1
    print(times)
    for key in ("calltree", "watch", "snapshot", "watch_keep_0"):
        assert all(math.isfinite(v) and v >= 0 for v in times[key].values()), (key, times[key])
    assert times["watch"]["emit_shards"] == 1 and times["watch_keep_0"]["emit_shards"] == 0
