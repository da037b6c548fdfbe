"""GPU tests of the snapshot of a prepared job (snap_reduce_kernel and snap_gather_kernel, and the call-tree pass in summary
mode over a prefix, through dvt_rv32_job_snapshot / Prover.job_snapshot, and `dvt_prover_host check --snapshot`).

Every case holds the device's answer against three things: the rule written over the independent model's rows and precompile
events (tests/_snapshot_ref.take), the model stopped at the position (agrees / state_at), and the host path
(capi.execute_snapshot at the same shard size), dict for dict.  Every comparison is of exact integers.
Shapes: bignum(40) at 2^14 cycles per shard is seven shards, four spans of 4096 records in each full one and a ragged last
shard of 4160 records (one span and one wave); at 2^10 every shard is smaller than a span; hammer offers one word from every
lane that has an access."""
import contextlib
import functools
import os
import subprocess

import pytest

from tests import _snapshot_ref as ref
from tests import guests
from tests.test_memory_host import CLI, ROOT
from tests.test_snapshot_host import accessed_words, call_guest, cli_block, deepest, page_ranges, tight_ranges
from tests.test_watch_host import hammer_slot, watched
from tests._watch_ref import _calls

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
EXIT = ref.EXIT


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


@contextlib.contextmanager
def _job_of(elf, stdin, log_shard, extra="", first=0, stride=1):
    """(snapshot(at, ranges, frames) on the prepared job of the guest, its number of shards)"""
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin), first=first, stride=stride)
    try:
        yield (lambda at, ranges=(), frames=64: p.job_snapshot(pk, job, at, ranges, frames)), p.job_shards(job)
    finally:
        p.job_free(job)
        p.pk_free(pk)
        p.close()


def _job(name, log_shard, extra="", first=0, stride=1):
    elf, stdin = watched(name)
    return _job_of(elf, stdin, log_shard, extra, first, stride)


@functools.lru_cache(maxsize=None)
def run_of(name, log_shard):
    elf, stdin = watched(name)
    return ref.model_run(elf, stdin, log_shard)


def without_ms(snap):
    return dict(snap, summary={k: v for k, v in snap["summary"].items() if k != "ms"})


def check(got, elf, stdin, log_shard, at, ranges, frames=64, where=""):
    """one device answer against the rule, the stopped model and the host path; returns the rule's answer"""
    from dvt_circuits_amd import capi

    run = ref.model_run(elf, stdin, log_shard)
    want = ref.take(run, at, ranges, frames)
    ref.same(got, want, where)
    ref.agrees(got, ref.state_at(elf, stdin, log_shard, want["summary"]["position"]), run, where)
    rc, rep, host, err = capi.execute_snapshot(elf, list(stdin), at, ranges, frames=frames, log_shard=log_shard)
    assert rc == 0 and without_ms(host) == without_ms(got), (where, err)
    return want


# ---------------------------------------------------------------- bignum(40) at 2^14: spans, shard edges, the ragged last shard
@pytest.fixture(scope="module")
def bignum():
    with _job("bignum", 14) as (snapshot, n):
        assert n == 7
        yield snapshot


BIGNUM_AT = [(1, 0), (1, 1), (2, 4095), (2, 4096), (2, 4097), (3, 0), (2, 16384), (7, 4096), (7, 4159), (7, 4160), EXIT]


@pytest.mark.parametrize("at", BIGNUM_AT)
def test_bignum_at_span_and_shard_edges(bignum, at):
    run = run_of("bignum", 14)
    assert run.cycles == 102464 and len(run.shards[-1]["rows"]) == 4160
    elf, stdin = watched("bignum")
    for ranges in (page_ranges(run), tight_ranges(run), ()):
        got = bignum(at, ranges)
        want = check(got, elf, stdin, 14, at, ranges, where="bignum at %s" % (at,))
        assert ref.no_value(got) == []
    s = got["summary"]
    print(at, s)
    if at == (1, 0):
        assert s["depth"] == 0 and all(c["flags"] == (1 if k else 0) for k, c in enumerate(got["regs"]))
    if at in ((7, 4160), EXIT):
        assert [c["value"] for c in got["regs"]] == run.reg and (s["position"], s["shard"], s["row"]) == (run.cycles, 7, 4160)
        full = bignum(at, tight_ranges(run))
        assert all(c["value"] == run.mem.get(c["addr"], 0) for c in full["words"] if not c["flags"] & ref.NO_VALUE)


def test_bignum_equal_positions_give_equal_answers(bignum):
    run = run_of("bignum", 14)
    ranges = tight_ranges(run)
    a, b = bignum((3, 0), ranges), bignum((2, 16384), ranges)
    assert without_ms(a) == without_ms(b) and a["summary"]["position"] == 2 * 16384 and (a["summary"]["shard"], a["summary"]["row"]) == (3, 0)
    a, b = bignum((7, 4160), ranges), bignum(EXIT, ranges)
    assert without_ms(a) == without_ms(b)


# ---------------------------------------------------------------- hammer: one word from every lane
def _hammer_case(log_shard):
    run = run_of("hammer", log_shard)
    slot = hammer_slot(run)
    accesses = [(sh["index"], i) for sh in run.shards for i, r in enumerate(sh["rows"]) if r.ins.kind in ("lw", "sw") and r.maddr & ~3 == slot]
    assert len(accesses) == 6000
    return run, slot, accesses, [(slot - 32, slot + 32)]


@pytest.mark.parametrize("log_shard", (14, 10))
def test_hammer_the_slot_and_its_frame(log_shard):
    run, slot, accesses, ranges = _hammer_case(log_shard)
    elf, stdin = watched("hammer")
    assert len(run.shards) == (2 if log_shard == 14 else 23)
    mid = accesses[3001]
    in_wave = next(a for a in accesses[2000:] if 8 <= a[1] % 64 <= 56)      # neighbouring lanes of one wave hold the winners
    places = [(1, 0), (1, 1), mid, (mid[0], mid[1] + 1), in_wave, (in_wave[0], in_wave[1] + 1), (mid[0], 0), (len(run.shards), 0), EXIT]
    with _job("hammer", log_shard) as (snapshot, n):
        assert n == len(run.shards)
        for at in places:
            got = snapshot(at, ranges)
            check(got, elf, stdin, log_shard, at, ranges, where="hammer at %s" % (at,))
            assert ref.no_value(got) == []
        # between a store of the slot and the load that follows it: the slot holds what was stored, from the record before
        got = snapshot((in_wave[0], in_wave[1] + 1), ranges)
        cell = next(c for c in got["words"] if c["addr"] == slot)
        assert (cell["shard"], cell["row"]) == in_wave and cell["flags"] & 2


def test_hammer_every_other_access_of_a_span():
    """64 positions in one span, each at an access of the slot: the winner before and the winner after move lane by lane"""
    run, slot, accesses, ranges = _hammer_case(14)
    elf, stdin = watched("hammer")
    span = [a for a in accesses if a[0] == 1 and 4096 <= a[1] < 8192]
    assert len(span) >= 128
    values = []
    with _job("hammer", 14) as (snapshot, n):
        for at in span[:128:2]:
            got = snapshot(at, ranges)
            check(got, elf, stdin, 14, at, ranges, where="hammer at %s" % (at,))
            values.append(next(c["value"] for c in got["words"] if c["addr"] == slot))
    assert len(set(values)) > 32      # (the counter in the slot moves on)


# ---------------------------------------------------------------- precompile calls and hints: NO_VALUE and INITIAL
@pytest.mark.parametrize("name", ("sha256_straddling", "curve_ops", "hint_sum"))
@pytest.mark.parametrize("log_shard", (10, 14))
def test_no_value_and_initial_are_the_references(name, log_shard):
    run = run_of(name, log_shard)
    elf, stdin = watched(name)
    ranges = tight_ranges(run)
    assert (len(run.shards) > 1) == (log_shard == 10)
    c = run.cycles
    calls = {(sh["index"], row) for sh in run.shards for row in _calls(sh)}
    seen = 0
    with _job(name, log_shard) as (snapshot, n):
        for at in [(1, 0), (1, 1), ref.locate(run, c // 3), ref.locate(run, c // 2), ref.locate(run, 3 * c // 4), EXIT]:
            for rg in (ranges, page_ranges(run)):
                got = snapshot(at, rg)
                want = check(got, elf, stdin, log_shard, at, rg, where="%s at %s" % (name, at))
                assert ref.no_value(got, False) == ref.no_value(want, False)
                assert [k["addr"] for k in got["words"] if k["flags"] & ref.INITIAL] == [k["addr"] for k in want["words"] if k["flags"] & ref.INITIAL]
            for cell in got["words"]:
                if cell["flags"] & ref.NO_VALUE and not cell["flags"] & ref.UNTOUCHED:
                    assert (cell["shard"], cell["row"]) in calls, cell      # a NO_VALUE cell names the call
            seen += len(ref.no_value(got))
            print(name, log_shard, at, "NO_VALUE", len(ref.no_value(got)), "of", len(accessed_words(run)), "accessed words; INITIAL", got["summary"]["initial"])
    if name == "sha256_straddling":
        assert seen > 0
    else:
        assert seen == 0


# ---------------------------------------------------------------- backtraces
@pytest.mark.parametrize("name", ("recurse", "stray", "tail"))
@pytest.mark.parametrize("log_shard", (10, 14))
def test_backtraces(name, log_shard):
    elf = call_guest(name)
    run = ref.model_run(elf, (), log_shard)
    deep, depth = deepest(run)
    c = run.cycles
    rows = [r for sh in run.shards for r in sh["rows"]]
    with _job_of(elf, (), log_shard) as (snapshot, n):
        assert n == len(run.shards)
        for g in sorted({0, 1, 2, c // 2, deep - 1, deep, deep + 1, c - 1, c}):
            at = ref.locate(run, g) if g < c else EXIT
            for frames in (8, 512):
                got = snapshot(at, (), frames)
                check(got, elf, (), log_shard, at, (), frames, "%s at %d frames %d" % (name, g, frames))
        got = snapshot(ref.locate(run, deep), (), 512)
        assert got["summary"]["depth"] == depth == len(got["frames"]) and got["frames"][-1]["call_pc"] == 0xFFFFFFFF
        for f in got["frames"][:-1]:      # call_pc and ra of every frame: the model's row before the frame opened
            opened = sum(len(sh["rows"]) for sh in run.shards[:f["open_shard"] - 1]) + f["open_row"]
            assert (f["call_pc"], f["ra"], f["fn_pc"]) == (rows[opened - 1].ins.pc, rows[opened - 1].a, rows[opened].ins.pc), f
        assert len(snapshot(ref.locate(run, deep), (), 8)["frames"]) == min(8, depth)
        if name == "stray":
            assert snapshot(EXIT)["summary"]["unmatched_returns"] == 1
    if name == "recurse":
        assert depth > 320 and (log_shard == 14 or len({f["open_shard"] for f in got["frames"]}) > 8)


# ---------------------------------------------------------------- range limits
def test_range_limits():
    from dvt_circuits_amd import capi

    run = run_of("bignum", 14)
    elf, stdin = watched("bignum")
    lo = min(accessed_words(run)) & ~4095
    sixteen = [(lo + 1024 * k, lo + 1024 * (k + 1)) for k in range(16)]      # 16 ranges, exactly 4096 words
    overlap = [(lo, lo + 256), (lo + 128, lo + 512), (lo, lo + 256)]
    with _job("bignum", 14) as (snapshot, n):
        for at in ((4, 5000), EXIT):
            got = snapshot(at, sixteen)
            assert got["summary"]["n_words"] == 4096 == len(got["words"])
            check(got, elf, stdin, 14, at, sixteen, where="sixteen ranges")
            got = snapshot(at, overlap)
            check(got, elf, stdin, 14, at, overlap, where="overlapping ranges")
            w = got["words"]
            assert w[32:64] == w[64:96] and w[:64] == w[160:224]
            got = snapshot(at, ())
            assert got["words"] == [] and got["summary"]["n_words"] == 0
            check(got, elf, stdin, 14, at, (), where="no ranges")
        with pytest.raises(capi.DvtError) as e:
            snapshot(EXIT, sixteen + [(lo, lo + 4)])
        assert e.value.code == capi.DVT_ERR_INPUT
        with pytest.raises(capi.DvtError) as e:
            snapshot(EXIT, [(lo, lo + 4 * 4097)])
        assert e.value.code == capi.DVT_ERR_INPUT


# ---------------------------------------------------------------- handles and jobs
def test_two_members_give_the_one_device_answer():
    for name, log_shard in (("bignum", 14), ("sha256_straddling", 10)):
        run = run_of(name, log_shard)
        elf, stdin = watched(name)
        ranges = tight_ranges(run)
        c = run.cycles
        places = [(1, 1), ref.locate(run, c // 3), (2, 0), ref.locate(run, 2 * c // 3), EXIT]
        with _job(name, log_shard) as (snapshot, n):
            one = [snapshot(at, ranges) for at in places]
        with _job(name, log_shard, ', "devices": [0, 0]') as (snapshot, n):
            two = [snapshot(at, ranges) for at in places]
            assert n == len(run.shards) > 1
        for at, a, b in zip(places, one, two):
            assert without_ms(a) == without_ms(b), at
            check(b, elf, stdin, log_shard, at, ranges, where="%s on two members at %s" % (name, at))


def test_a_partial_job_is_refused():
    from dvt_circuits_amd import capi

    for first in (0, 1):
        with _job("bignum", 14, first=first, stride=2) as (snapshot, n):
            with pytest.raises(capi.DvtError) as e:
                snapshot(EXIT)
            assert e.value.code == capi.DVT_ERR_UNSUPPORTED


@pytest.mark.parametrize("extra", ["", ', "keep_phase1": 0'])
def test_the_job_is_left_as_found(extra):
    """the proof of a job that was snapshotted before and after proving equals that of a job that never was"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    run = ref.model_run(elf, (), 11)
    ranges = tight_ranges(run)
    places = [(2, 100), EXIT]
    proofs = []
    for inspect in (True, False):
        p = _prover(11, extra)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = [p.job_snapshot(pk, job, at, ranges) for at in places] if inspect else None
        proofs.append(p.prove_job(pk, job))
        if inspect:
            after = [p.job_snapshot(pk, job, at, ranges) for at in places]
            assert [without_ms(s) for s in before] == [without_ms(s) for s in after]
            assert p.prove_job(pk, job) == proofs[0]
            for at, got in zip(places, before):
                check(got, elf, (), 11, at, ranges, where="commit_only at %s" % (at,))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why


def test_a_snapshot_drains_a_running_pipeline():
    """two lanes, prove_shard of shard 0 starts the phase-2 pipeline, the snapshot stops it and is correct; the shards proven
    afterwards assemble into the container of a handle that never asked"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    run = ref.model_run(elf, (), 11)
    ranges = tight_ranges(run)
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
            check(p.job_snapshot(pk, job, (3, 7), ranges), elf, (), 11, (3, 7), ranges, where="after prove_shard(0)")
        proofs += [p.prove_shard(pk, job, i, ch) for i in range(1, n)]
        containers.append(p.assemble(job, proofs))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert containers[0] == containers[1]
    ok, ec, pv, why = capi.verify(vk, containers[0], Q, POW)
    assert ok and pv == b"check me", why


def test_the_times_of_a_call():
    elf, stdin = watched("bignum")
    p = _prover(14)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin))
    p.job_snapshot(pk, job, (4, 5000), tight_ranges(run_of("bignum", 14)))
    t = p.job_snapshot_times()
    print(t)
    assert sorted(t) == ["backtrace_ms", "gather_ms", "reduce_ms"] and all(0 < v < 1000 for v in t.values()), t
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_cli_check_snapshot(tmp_path):
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(example, "rb").read())
    run = ref.model_run(elf, (buf,))
    lo, hi = tight_ranges(run)[0]
    hi = min(hi, lo + 64)
    want = ref.take(run, EXIT, [(lo, hi)], 16)
    base = [CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path)]
    r = subprocess.run(base + ["--snapshot", "exit", "--dump", "0x%x+%d" % (lo, hi - lo)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ") and r.stdout.splitlines()[1].startswith("snapshot: ")
    summary, regs, frames, words = cli_block(r.stdout)
    s = want["summary"]
    assert summary == dict({k: s[k] for k in ("position", "cycles", "shard", "row", "pc", "depth", "unmatched_returns", "no_value", "initial", "untouched")},
                           frames=s["n_frames"], words=s["n_words"])
    assert regs == {capi.REG_NAMES[k]: want["regs"][k]["value"] for k in range(1, 32)} and regs["sp"] == run.reg[2]
    assert [int(f[1], 16) for f in frames] == [f["fn_pc"] for f in want["frames"]]
    assert words == {c["addr"]: "??" if c["flags"] & ref.NO_VALUE else "%08x" % c["value"] for c in want["words"]}
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith("clean: ") and len(plain.stdout.splitlines()) == 1
