"""GPU tests of the memory report of a prepared job (memory_records_kernel and memory_gather_kernel through
dvt_rv32_job_memory / Prover.job_memory, and `dvt_prover_host check --show-memory`).

The yardstick is the rule written over the independent model's rows and precompile events (tests/_memory_ref.py); the host
path (capi.execute_memory) must say the same.  Every comparison is of exact integers.  Shapes: bignum(40) at 2^14 cycles per
shard is seven shards, four workgroups in each full one and a ragged last shard of 4160 records; at 2^10 every shard is smaller
than a workgroup's span of 4096 records; the guests of tests/guests_memory.py store to more pages inside one span than the LDS
page cache has slots, hammer one stack slot from every lane, and set all bits of one bitmap word and its neighbours; the SHA
guest's arrays straddle a page."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import _memory_ref as ref
from tests import guests
from tests.test_memory_host import CLI, ROOT, SUMMARY_KEYS, block_of, guest, ranges_of

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
COUNTERS = ("cycles", "loads", "stores", "pre_reads", "pre_writes", "pre_calls", "first_touches", "sp_writes")


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


def _job_memory(name, log_shard, extra="", first=0, stride=1):
    elf, stdin = guest(name)
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin), first=first, stride=stride)
    mem = p.job_memory(pk, job)
    n = p.job_shards(job)
    p.job_free(job)
    p.pk_free(pk)
    p.close()
    return mem, n


@functools.lru_cache(maxsize=None)
def _run(name, log_shard=21):
    elf, stdin = guest(name)
    return ref.model_run(elf, stdin, log_shard)


@functools.lru_cache(maxsize=None)
def _want(name):
    return ref.report(_run(name))


@functools.lru_cache(maxsize=None)
def _host(name):
    from dvt_circuits_amd import capi

    elf, stdin = guest(name)
    rc, rep, mem, err = capi.execute_memory(elf, list(stdin))
    assert rc == 0, err
    return mem


def _same(a, b, shards=True):
    """two reports say the same (everything but the time, and the shard counts when the shard sizes differ)"""
    sa, sb = dict(a["summary"], ms=0), dict(b["summary"], ms=0)
    if not shards:
        for k in ("shards_tallied", "shards_total"):
            sa[k] = sb[k] = 0
    assert sa == sb, sorted(set(sa.items()) ^ set(sb.items()))
    assert np.array_equal(a["first_touch"], b["first_touch"]) and a["pages"] == b["pages"]


@pytest.mark.parametrize("name, log_shard", [("bignum", 14), ("subword", 10), ("hint_sum", 10), ("many_pages", 14), ("hammer", 14), ("bit_edges", 14),
                                             ("sha256_straddling", 14), ("curve_ops", 14), ("u256_ops", 14)])
def test_job_memory_is_the_models_and_the_hosts(name, log_shard):
    mem, n = _job_memory(name, log_shard)
    s = mem["summary"]
    print(name, log_shard, s)
    run = _run(name, log_shard)
    assert n == len(run.shards) == s["shards_total"] == s["shards_tallied"]
    ref.same_report(mem, _want(name), "%s at 2^%d" % (name, log_shard), shards=False)
    _same(mem, _host(name), shards=False)
    if name == "bignum":
        assert n == 7 and s["cycles"] == 102464 and len(run.shards[-1]["rows"]) == 4160
    if name in ("subword", "hint_sum"):
        assert n > 1 and all(len(sh["rows"]) <= 1024 for sh in run.shards)
    if name == "many_pages":
        from dvt_circuits_amd import capi

        assert n == 1 and s["n_pages"] > capi.MEMORY_LDS_PAGE_SLOTS


def test_shard_size_does_not_change_the_report():
    small, n_small = _job_memory("arith", 10)
    large, n_large = _job_memory("arith", 14)
    assert n_small > 1 and n_large == 1
    _same(small, large, shards=False)
    ref.same_report(small, _want("arith"), "arith", shards=False)


def test_partial_jobs_add_up_to_the_whole():
    run = _run("bignum", 14)
    odd, n = _job_memory("bignum", 14, first=1, stride=2)
    even, _ = _job_memory("bignum", 14, first=0, stride=2)
    whole, _ = _job_memory("bignum", 14)
    assert n == 7 and (odd["summary"]["shards_tallied"], even["summary"]["shards_tallied"], odd["summary"]["shards_total"]) == (3, 4, 7)
    ref.same_report(odd, ref.report(run, [1, 3, 5]), "shards 1, 3, 5")
    ref.same_report(even, ref.report(run, [0, 2, 4, 6]), "shards 0, 2, 4, 6")
    for k in COUNTERS:
        assert odd["summary"][k] + even["summary"][k] == whole["summary"][k], k
    assert np.array_equal(odd["first_touch"] + even["first_touch"], whole["first_touch"])
    assert max(odd["summary"]["words"], even["summary"]["words"]) <= whole["summary"]["words"] <= odd["summary"]["words"] + even["summary"]["words"]
    assert odd["summary"]["mem_init_rows"] == even["summary"]["mem_init_rows"] == 0 and whole["summary"]["mem_init_rows"] == len(run.mem_rows())
    by_page = {}
    for pg in odd["pages"] + even["pages"]:
        sums = by_page.setdefault(pg["page"], dict.fromkeys(("loads", "stores", "first", "pre_reads", "pre_writes"), 0))
        for k in sums:
            sums[k] += pg[k]
    assert by_page == {pg["page"]: {k: pg[k] for k in by_page[pg["page"]]} for pg in whole["pages"]}


def test_two_members_give_the_one_device_report():
    one, _ = _job_memory("bignum", 14)
    two, n = _job_memory("bignum", 14, ', "devices": [0, 0]')
    assert n == 7
    _same(one, two)
    one, _ = _job_memory("sha256_straddling", 10)
    two, n = _job_memory("sha256_straddling", 10, ', "devices": [0, 0]')
    assert n > 1
    _same(one, two)


@pytest.mark.parametrize("extra", ["", ', "keep_phase1": 0'])
def test_the_job_is_left_as_found(extra):
    """the proof of a job that was inspected before and after proving equals that of a job that never was"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    proofs = []
    for inspect in (True, False):
        p = _prover(11, extra)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = p.job_memory(pk, job) if inspect else None
        proofs.append(p.prove_job(pk, job))
        if inspect:
            _same(before, p.job_memory(pk, job))
            assert p.prove_job(pk, job) == proofs[0]
            ref.same_report(before, ref.report(ref.model_run(elf, (), 11)), "commit_only")
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why


def test_a_report_drains_a_running_pipeline():
    """two lanes, prove_shard of shard 0 starts the phase-2 pipeline, the report stops it; the shards proven afterwards assemble
    into the container of a handle that never asked"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    containers = []
    for inspect in (True, False):
        p = _prover(11, ', "lanes": 2')
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        n = p.job_shards(job)
        assert n == 3
        headers = [p.commit_shard(pk, job, i) for i in range(n)]
        ch = capi.rv32_challenges(vk, headers)
        proofs = [p.prove_shard(pk, job, 0, ch)]
        if inspect:
            ref.same_report(p.job_memory(pk, job), ref.report(ref.model_run(elf, (), 11)), "after prove_shard(0)")
        proofs += [p.prove_shard(pk, job, i, ch) for i in range(1, n)]
        containers.append(p.assemble(job, proofs))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert containers[0] == containers[1]
    ok, ec, pv, why = capi.verify(vk, containers[0], Q, POW)
    assert ok and pv == b"check me", why


def test_cli_check_show_memory(tmp_path):
    elf = guests.commit_only(b"check me")
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    want = ref.report(ref.model_run(elf))
    base = [CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path)]
    r = subprocess.run(base + ["--show-memory"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ") and r.stdout.splitlines()[1].startswith("memory: ")
    summary, ranges = block_of(r.stdout)
    assert summary == dict({k: want["summary"][k] for k in SUMMARY_KEYS}, pages=want["summary"]["n_pages"])
    assert ranges == ranges_of(want["pages"])
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith("clean: ") and len(plain.stdout.splitlines()) == 1
