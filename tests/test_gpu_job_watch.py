"""GPU tests of the watchpoint search of a prepared job (watch_count_kernel, watch_scan_kernel and watch_emit_kernel through
dvt_rv32_job_watch / Prover.job_watch, and `dvt_prover_host check --watch`).

The yardstick is the rule written over the independent model's rows and precompile events (tests/_watch_ref.py); the host
path (capi.execute_watch at the same shard size) must say the same.  Every comparison is of exact integers and whole hit lists.
Shapes: bignum(40) at 2^14 cycles per shard is seven shards, four spans of 4096 records in each full one and a ragged last
shard of 4160 records (one span and one wave); at 2^10 every shard is smaller than a span; hammer hits one word from every
lane that has an access."""
import collections
import contextlib
import functools
import os
import subprocess

import pytest

from tests import _watch_ref as ref
from tests import guests
from tests.test_memory_host import CLI, ROOT
from tests.test_watch_host import cli_line, cli_totals, hammer_slot, host_watch, rows_of, run_of, standard_queries, watched
from tools import watch_guest

pytestmark = pytest.mark.gpu
Q, POW = 6, 5


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


@contextlib.contextmanager
def _job(name, log_shard, extra="", first=0, stride=1):
    """(search(queries, keep) on the prepared job of the guest, its number of shards)"""
    elf, stdin = watched(name)
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin), first=first, stride=stride)
    try:
        yield (lambda queries, keep: p.job_watch(pk, job, queries, keep=keep)), p.job_shards(job)
    finally:
        p.job_free(job)
        p.pk_free(pk)
        p.close()


@functools.lru_cache(maxsize=None)
def _want(name, log_shard):
    run = run_of(name, log_shard)
    return ref.search(run, standard_queries(run))


@pytest.mark.parametrize("name, log_shard", [("arith", 14), ("subword", 14), ("hint_sum", 14), ("bignum", 14), ("hammer", 14), ("sha256_straddling", 14),
                                             ("curve_ops", 14), ("u256_ops", 14), ("sub_stores", 14), ("subword", 10), ("hint_sum", 10)])
def test_job_watch_is_the_models_and_the_hosts(name, log_shard):
    run = run_of(name, log_shard)
    queries, want = standard_queries(run), _want(name, log_shard)
    print(name, log_shard, [w["total"] for w in want])
    with _job(name, log_shard) as (search, n):
        assert n == len(run.shards)
        for keep in (5, 256):
            got = search(queries, keep)
            ref.same(got, want, keep, "%s at 2^%d keep %d" % (name, log_shard, keep))
            assert got == host_watch(name, queries, keep, log_shard=log_shard)
        assert [g["total"] for g in search(queries, 0)] == [w["total"] for w in want]
    if name == "bignum":
        assert n == 7 and run.cycles == 102464 and len(run.shards[-1]["rows"]) == 4160
    if log_shard == 10:
        assert n > 1 and all(len(sh["rows"]) <= 1024 for sh in run.shards)


def _pos(h):
    return h["shard"], h["row"]


@pytest.mark.parametrize("keep", [1, 63, 64, 65, 256])
def test_kept_ranges_at_every_boundary(keep):
    """An instruction of bignum's inner loop (a hit every 18 records or so: 256 of them cross a span boundary) and the whole
    text (a hit in every lane: a kept range of 63, 64, 65 ends inside a wave, at its edge, in the next one), whole and through
    windows that end in the ragged last shard, hold 2 keep - 1 hits, hold none, or begin and end in the middle of a span."""
    from dvt_circuits_amd import capi

    run = run_of("bignum", 14)
    rows = rows_of(run)
    hot = collections.Counter(r.ins.pc for _, _, r in rows).most_common(1)[0][0]
    text = (run.text_base, run.text_base + 4 * run.n_instr)
    at = [(s, i) for s, i, r in rows if r.ins.pc == hot]
    units, spans = {(s, i // 64) for s, i in at}, {(s, i // 4096) for s, i in at}
    print("hits of 0x%x: %d, in %d of %d waves, %d of %d spans" % (hot, len(at), len(units), len({(s, i // 64) for s, i, _ in rows}), len(spans),
                                                                 len({(s, i // 4096) for s, i, _ in rows})))
    # (the loop ends in the sixth shard: the instruction has hits in 23 of the 26 spans; the whole text hits every lane of all)
    assert {s for s, _ in at} == set(range(1, 7)) and len(spans) == 23 and len(units) > 1400
    a = 1000
    queries = [
        capi.watch_pc(hot),
        capi.watch_pc(*text),
        capi.watch_pc(*text, window=((0, 0), (7, 100))),                         # the last list crosses from shard 6 into the ragged shard
        capi.watch_pc(*text, window=((0, 0), (7, 64))),                          # ... and ends at a wave edge of it
        capi.watch_pc(hot, window=(at[a], at[a + 2 * keep - 1])),                # 2 keep - 1 hits: the lists overlap in one hit
        capi.watch_pc(hot, window=((at[a][0], at[a][1] + 1), at[a + 1])),        # between two hits: none
        capi.watch_pc(hot, window=((2, 5000), (4, 9000))),                       # from and to in the middle of a span
        capi.watch_pc(*text, window=((2, 4096 - 100), (2, 4096 + keep))),        # the first list crosses a span boundary of the dense query
        capi.watch_pc(*text, window=((3, 16384 - 30), (4, 40))),                 # a window across two full shards
        capi.watch_pc(*text, window=((7, 4096), (7, 4160))),                     # the last wave of the job
    ]
    want = ref.search(run, queries)
    assert want[4]["total"] == 2 * keep - 1 and want[5]["total"] == 0 and want[9]["total"] == 64 and want[8]["total"] == 70
    assert want[2]["total"] == 6 * 16384 + 100 and want[1]["total"] == run.cycles
    with _job("bignum", 14) as (search, n):
        got = search(queries, keep)
    ref.same(got, want, keep, "keep %d" % keep)
    assert got[4]["first"][-1] == got[4]["last"][0] and len(got[4]["first"]) == keep
    assert got[5] == dict(total=0, first=[], last=[])
    if keep == 256:
        assert _pos(got[2]["last"][0]) == (6, 16384 - 156) and _pos(got[2]["last"][-1]) == (7, 99)
        assert got[6]["first"][0]["row"] // 4096 < got[6]["first"][-1]["row"] // 4096      # the sparse query's first list crosses a span boundary
        assert got[6]["last"][0]["row"] // 4096 < got[6]["last"][-1]["row"] // 4096
    assert got == host_watch("bignum", queries, keep, log_shard=14)


def test_hammer_one_word_from_every_lane():
    from dvt_circuits_amd import capi

    run = run_of("hammer", 14)
    slot = hammer_slot(run)
    sp_values = collections.Counter(r.a for _, _, r in rows_of(run) if r.ins.rd == 2)
    low = min(v for v, n in sp_values.items() if n >= 3000)      # (sp inside the frame; li sp wrote two other values once)
    queries = [capi.watch_mem(slot, flags=capi.DVT_WATCH_STORE), capi.watch_mem(slot, flags=capi.DVT_WATCH_LOAD), capi.watch_reg(2, value=low),
               capi.watch_reg(2, value=low & 0xFF0, mask=0xFF0), capi.watch_reg(2), capi.watch_mem(slot, flags=capi.DVT_WATCH_LOAD | capi.DVT_WATCH_STORE)]
    want = ref.search(run, queries)
    assert [w["total"] for w in want[:3]] == [3000, 3000, 3000] and want[4]["total"] == 6002 and want[5]["total"] == 6000
    assert len(run.shards) == 2
    with _job("hammer", 14) as (search, n):
        for keep in (256, 7):
            got = search(queries, keep)
            ref.same(got, want, keep, "hammer keep %d" % keep)
            assert got == host_watch("hammer", queries, keep, log_shard=14)
        # the order is the execution's: stores and loads of the slot alternate, and every access points at the one before
        both = search(queries[5:], 256)[0]
        for part in ("first", "last"):
            flags = [h["flags"] for h in both[part]]
            assert flags[0] != flags[1] and flags == (flags[:2] * 128)
            for older, newer in zip(both[part], both[part][1:]):
                assert (newer["prev_shard"], newer["prev_clk"]) == (older["shard"], 4 * older["row"] + 6)
        # the history of the slot from the device, as the tool walks it
        hits, why = watch_guest.history(search, slot)
    model = [(s, i) for s, i, r in rows_of(run) if r.ins.kind in ("lw", "sw") and r.maddr & ~3 == slot]
    assert why == "first touch of the word" and [_pos(h) for h in hits] == model[::-1]


def _sixteen(run):
    from dvt_circuits_amd import capi

    queries = standard_queries(run)
    rows = rows_of(run)
    by_pc = collections.Counter(r.ins.pc for _, _, r in rows).most_common(4)
    return queries + [capi.watch_pc(pc, window=((2, 100), (6, 5000))) for pc, _ in by_pc]


def test_sixteen_queries_are_sixteen_calls():
    run = run_of("bignum", 14)
    queries = _sixteen(run)
    assert len(queries) == 16
    want = ref.search(run, queries)
    with _job("bignum", 14) as (search, n):
        together = search(queries, 9)
        alone = [search([q], 9)[0] for q in queries]
    ref.same(together, want, 9, "sixteen")
    for qi, one in enumerate(alone):
        for part in ("first", "last"):
            for h in one[part]:
                assert h["query"] == 0
                h["query"] = qi
    assert together == alone


def test_partial_jobs_find_the_hits_of_their_shards():
    run = run_of("bignum", 14)
    queries = standard_queries(run)
    with _job("bignum", 14, first=1, stride=2) as (search, n):
        odd = search(queries, 256)
        assert n == 7
    with _job("bignum", 14, first=0, stride=2) as (search, n):
        even = search(queries, 256)
    with _job("bignum", 14) as (search, n):
        whole = search(queries, 256)
    ref.same(odd, ref.search(run, queries, [1, 3, 5]), 256, "shards 2, 4, 6")
    ref.same(even, ref.search(run, queries, [0, 2, 4, 6]), 256, "shards 1, 3, 5, 7")
    assert {h["shard"] for g in odd for h in g["first"] + g["last"]} <= {2, 4, 6} and {h["shard"] for g in even for h in g["first"] + g["last"]} <= {1, 3, 5, 7}
    assert {h["shard"] for h in even[0]["last"]} == {7} and {h["shard"] for h in odd[0]["last"]} == {6}
    assert [a["total"] + b["total"] for a, b in zip(odd, even)] == [w["total"] for w in whole]


def test_two_members_give_the_one_device_answer():
    for name, log_shard in (("bignum", 14), ("sha256_straddling", 10)):
        run = run_of(name, log_shard)
        queries = standard_queries(run)
        with _job(name, log_shard) as (search, n):
            one = search(queries, 256)
        with _job(name, log_shard, ', "devices": [0, 0]') as (search, n):
            two = search(queries, 256)
            assert n == len(run.shards) > 1
        assert one == two
        ref.same(two, ref.search(run, queries), 256, name)


@pytest.mark.parametrize("extra", ["", ', "keep_phase1": 0'])
def test_the_job_is_left_as_found(extra):
    """the proof of a job that was searched before and after proving equals that of a job that never was"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    run = ref.model_run(elf, (), 11)
    queries = standard_queries(run)
    proofs = []
    for inspect in (True, False):
        p = _prover(11, extra)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = p.job_watch(pk, job, queries, keep=32) if inspect else None
        proofs.append(p.prove_job(pk, job))
        if inspect:
            assert before == p.job_watch(pk, job, queries, keep=32)
            assert p.prove_job(pk, job) == proofs[0]
            ref.same(before, ref.search(run, queries), 32, "commit_only")
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why


def test_a_search_drains_a_running_pipeline():
    """two lanes, prove_shard of shard 0 starts the phase-2 pipeline, the search stops it and is correct; the shards proven
    afterwards assemble into the container of a handle that never asked"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    run = ref.model_run(elf, (), 11)
    queries = standard_queries(run)
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
            ref.same(p.job_watch(pk, job, queries, keep=32), ref.search(run, queries), 32, "after prove_shard(0)")
        proofs += [p.prove_shard(pk, job, i, ch) for i in range(1, n)]
        containers.append(p.assemble(job, proofs))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert containers[0] == containers[1]
    ok, ec, pv, why = capi.verify(vk, containers[0], Q, POW)
    assert ok and pv == b"check me", why


def test_cli_check_watch(tmp_path):
    elf = guests.commit_only(b"check me")
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    run = ref.model_run(elf)
    hot = collections.Counter(r.ins.pc for _, _, r in rows_of(run)).most_common(1)[0][0]
    specs = ["pc:0x%x" % hot, "reg:t0", "mem:0+0x38000000", "store:0+0x38000000", "pread:0+0x38000000"]
    want = ref.search(run, [watch_guest.parse_spec(s) for s in specs])
    base = [CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path)]
    r = subprocess.run(base + [x for s in specs for x in ("--watch", s)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ") and r.stdout.splitlines()[1].startswith("watch ")
    totals, lines = cli_totals(r.stdout)
    assert totals == {s: w["total"] for s, w in zip(specs, want)} and all(w["total"] for w in want[:4])
    for s, w in zip(specs, want):
        assert lines[s] == [cli_line(h) for h in w["hits"][-4:]], s
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith("clean: ") and len(plain.stdout.splitlines()) == 1
