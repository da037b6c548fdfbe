"""GPU tests of the origin slice of a prepared job (origin_reduce_kernel and origin_gather_kernel through dvt_rv32_job_origin /
Prover.job_origin, and `dvt_prover_host check --origin`).

Every case holds the device's answer against four things: the rule written over the independent model's rows and precompile
events (tests/_origin_ref.slice_of), the two yardsticks that do not depend on the rule (edges_agree: the producer's record
holds what the consumer's record read; root_agrees: the root's value is the stopped model's), and the host path
(capi.execute_origin at the same shard size), dict for dict.  summary.passes is the sum over the reference's levels of
ceil(questions / 256).  Every comparison is of exact integers, and every property of a shape is asserted on the reference's
answer inside the test.
Shapes: bignum(40) at 2^14 cycles per shard is seven shards, four spans of 4096 records in each full one and a ragged last
shard of 4160 records; at 2^10 every shard is smaller than a span."""
import contextlib
import functools
import os
import subprocess

import pytest

from tests import _origin_ref as ref
from tests import guests
from tests.test_memory_host import CLI, ROOT
from tests.test_origin_host import cli_agrees, last_words
from tests.test_watch_host import hammer_slot, watched

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
EXIT = ref.EXIT
A0, A1, A3 = (ref.REG, 10), (ref.REG, 11), (ref.REG, 13)


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


@contextlib.contextmanager
def _job_of(elf, stdin, log_shard, extra="", first=0, stride=1):
    """(origin(at, target, **kw) on the prepared job of the guest, its number of shards, the prover)"""
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin), first=first, stride=stride)
    origin = lambda at, target, **kw: p.job_origin(pk, job, at, target, **kw)
    origin.p, origin.pk, origin.job = p, pk, job
    try:
        yield origin, p.job_shards(job), p
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


def without_ms(got, passes=None):
    s = {k: v for k, v in got["summary"].items() if k != "ms"}
    if passes is not None:
        s["passes"] = passes
    return dict(got, summary=s)


def check(got, elf, stdin, log_shard, at, target, where="", **kw):
    """one device answer against the rule, both yardsticks and the host path; returns the rule's answer"""
    from dvt_circuits_amd import capi

    run = ref.model_run(elf, stdin, log_shard)
    want = ref.slice_of(run, at, target, kw.get("follow_addr", False), kw.get("depth", ref.MAX_DEPTH), kw.get("nodes", ref.MAX_NODES),
                        kw.get("edges", ref.MAX_EDGES))
    ref.same(got, want, where=where)
    assert got["summary"]["passes"] == sum(-(-q // 256) for q in want["level_questions"]), where
    ref.edges_agree(got, where)
    ref.root_agrees(got, target, ref.state_at(elf, stdin, log_shard, want["summary"]["position"]), where)
    rc, rep, host, err = capi.execute_origin(elf, list(stdin), at, target, log_shard=log_shard, **kw)
    assert rc == 0 and without_ms(host) == without_ms(got, passes=0), (where, err)
    return want


# ---------------------------------------------------------------- bignum(40) at 2^14: spans, shard edges, chunks, the node cap
@pytest.fixture(scope="module")
def bignum():
    with _job("bignum", 14) as (origin, n, p):
        assert n == 7
        yield origin


def test_bignum_a1_at_exit_fills_the_node_cap(bignum):
    run = run_of("bignum", 14)
    assert run.cycles == 102464 and len(run.shards[-1]["rows"]) == 4160
    elf, stdin = watched("bignum")
    got = bignum(EXIT, A1)
    want = check(got, elf, stdin, 14, EXIT, A1, "bignum a1 at exit")
    s = want["summary"]
    print(s, "widest level", max(want["level_questions"]))
    assert s["n_nodes"] == 1024 and s["cut"] > 0 and all(e["to"] == ref.NONE and e["src_shard"] for e in want["edges"] if e["flags"] & ref.CUT)
    assert len({n["shard"] for n in want["nodes"]}) >= 2 and len(ref.spans_of(want)) >= 3
    assert max(want["level_questions"]) > 256 and s["passes"] > s["levels"]      # a level of two chunks
    assert got["summary"]["passes"] == s["passes"]


@pytest.mark.parametrize("at", [(2, 4095), (2, 4096), (3, 0), (7, 4160)])
def test_bignum_at_span_and_shard_edges(bignum, at):
    run = run_of("bignum", 14)
    elf, stdin = watched("bignum")
    g = ref.global_of(run, at)
    for target in [A0, A1] + [(ref.WORD, a) for a in last_words(run, g, 2)]:
        for follow in (False, True):
            got = bignum(at, target, follow_addr=follow)
            check(got, elf, stdin, 14, at, target, "bignum %s at %s follow %s" % (target, at, follow), follow_addr=follow)
    if at == (7, 4160):
        assert without_ms(bignum(at, A1)) == without_ms(bignum(EXIT, A1))


def test_bignum_small_shards():
    """2^10: every shard is smaller than a span, and the slice spans at least five shards"""
    run = run_of("bignum", 10)
    elf, stdin = watched("bignum")
    assert len(run.shards) == 101 and all(len(sh["rows"]) <= 1024 for sh in run.shards)
    with _job("bignum", 10) as (origin, n, p):
        assert n == 101
        for at, target in ((EXIT, A1), (ref.locate(run, run.cycles // 2), (ref.REG, 6))):
            want = check(origin(at, target), elf, stdin, 10, at, target, "bignum 2^10 %s at %s" % (target, at))
            assert len({n["shard"] for n in want["nodes"]}) >= 5, at


# ---------------------------------------------------------------- calls, leaves, depth
def test_u256_ops_calls_leaves_and_the_depth_limit():
    run = run_of("u256_ops", 10)
    elf, stdin = watched("u256_ops")
    at = ref.locate(run, run.cycles // 2)
    with _job("u256_ops", 10) as (origin, n, p):
        assert n == len(run.shards) > 1
        got = origin(at, A3)
        want = check(got, elf, stdin, 10, at, A3, "u256_ops a3 from the middle")
        calls = [n for n in want["nodes"] if n["kind"] == ref.CALL]
        assert calls and all(n["n_edges"] >= 16 for n in calls)
        for n in calls:
            assert all(e["role"] == ref.MEM and e["flags"] & ref.NO_VALUE for e in want["edges"][n["first_edge"]:n["first_edge"] + n["n_edges"]])
        leaves = [e for e in want["edges"] if e["flags"] & ref.INITIAL]
        assert leaves and any(e["flags"] & ref.IMAGE for e in leaves)
        assert any(n["flags"] & ref.UNEXPANDED and n["depth"] == 64 for n in want["nodes"]) and want["summary"]["depth"] == 64
        print("calls", len(calls), "leaves", len(leaves), "unexpanded", want["summary"]["unexpanded"])
        check(origin(at, A3, follow_addr=True), elf, stdin, 10, at, A3, "u256_ops a3 with addresses", follow_addr=True)


def test_hammer_a_chain_across_a_shard_edge():
    run = run_of("hammer", 10)
    elf, stdin = watched("hammer")
    at = ref.locate(run, run.cycles // 2)
    with _job("hammer", 10) as (origin, n, p):
        want = check(origin(at, A0), elf, stdin, 10, at, A0, "hammer a0 from the middle")
        assert max(want["level_questions"]) == 1 and want["summary"]["n_nodes"] == 65      # one node per level
        assert len({n["shard"] for n in want["nodes"]}) >= 2
        slot = (ref.WORD, hammer_slot(run))
        for follow in (False, True):
            check(origin(at, slot, follow_addr=follow), elf, stdin, 10, at, slot, "hammer's slot", follow_addr=follow)


def test_sub_stores_mem_edges_out_of_store_nodes():
    run = run_of("sub_stores", 10)
    elf = watched("sub_stores")[0]
    subs = [(sh["index"], i, r) for sh in run.shards for i, r in enumerate(sh["rows"]) if r.ins.kind in ("sb", "sh")]
    assert len(subs) == 7
    with _job("sub_stores", 10) as (origin, n, p):
        for shard, row, r in subs:
            target = (ref.WORD, r.maddr & ~3)
            want = check(origin((shard, row + 1), target), elf, (), 10, (shard, row + 1), target, "sub_stores at %d:%d" % (shard, row))
            first = want["nodes"][0]
            ins = want["edges"][first["first_edge"]:first["first_edge"] + first["n_edges"]]
            assert first["kind"] == ref.F_STORE and [e["value"] for e in ins if e["role"] == ref.MEM] == [r.m_prev]
        check(origin(EXIT, A1, follow_addr=True), elf, (), 10, EXIT, A1, "sub_stores a1 at exit", follow_addr=True)


def test_caps_depth_zero_and_an_unwritten_target(bignum):
    run = run_of("bignum", 14)
    elf, stdin = watched("bignum")
    full = ref.slice_of(run, EXIT, A1)
    wide = next(k for k, q in enumerate(full["level_questions"]) if q >= 8)
    cap = sum(full["level_questions"][:wide]) + full["level_questions"][wide] // 2
    want = check(bignum(EXIT, A1, edges=cap), elf, stdin, 14, EXIT, A1, "cap_edges stops mid-level", edges=cap)
    assert want["summary"]["n_edges"] <= cap and want["summary"]["levels"] == wide + 1 and want["summary"]["unexpanded"] > 0
    assert len({n["depth"] for n in want["nodes"] if n["flags"] & ref.UNEXPANDED}) == 2
    want = check(bignum(EXIT, A1, depth=0), elf, stdin, 14, EXIT, A1, "depth 0", depth=0)
    assert len(want["nodes"]) == 1 and want["nodes"][0]["flags"] == ref.UNEXPANDED and len(want["edges"]) == 1
    want = check(bignum(EXIT, A1, nodes=0), elf, stdin, 14, EXIT, A1, "no nodes", nodes=0)
    assert want["edges"][0]["flags"] == ref.CUT and want["nodes"] == []
    want = check(bignum((4, 5000), A1, depth=7, nodes=50), elf, stdin, 14, (4, 5000), A1, "depth 7, 50 nodes", depth=7, nodes=50)
    quiet = next(k for k in range(31, 0, -1) if not any(r.ins.rd == k for sh in run.shards for r in sh["rows"]))
    for target in ((ref.REG, quiet), (ref.WORD, guests.HEAP + 0x100000)):
        want = check(bignum(EXIT, target), elf, stdin, 14, EXIT, target, "a target nothing wrote")
        assert want["nodes"] == [] and want["edges"][0]["flags"] & ref.INITIAL
    # nothing ran before (1, 0)
    want = check(bignum((1, 0), A1), elf, stdin, 14, (1, 0), A1, "before the first record")
    assert want["nodes"] == [] and want["summary"]["position"] == 0


def test_the_root_is_the_snapshots_writer(bignum):
    from dvt_circuits_amd import capi

    p, pk, job = bignum.p, bignum.pk, bignum.job
    for at in ((4, 5000), EXIT):
        snap = p.job_snapshot(pk, job, at)
        for k in (1, 2, 10, 11, 15):
            got = p.job_origin(pk, job, at, capi.origin_reg(k), depth=0)
            cell, root = snap["regs"][k], got["edges"][0]
            assert root["value"] == cell["value"] and (root["src_shard"], root["src_row"]) == (cell["shard"], cell["row"]), (at, k)
            if got["nodes"]:
                assert (got["nodes"][0]["shard"], got["nodes"][0]["row"], got["nodes"][0]["pc"]) == (cell["shard"], cell["row"], cell["pc"])
            else:
                assert cell["flags"] & capi.DVT_SNAP_INITIAL and root["flags"] & ref.INITIAL


# ---------------------------------------------------------------- handles and jobs
def test_two_members_give_the_one_device_answer(bignum):
    run = run_of("bignum", 14)
    elf, stdin = watched("bignum")
    places = [((2, 4096), A1, False), (EXIT, A1, True), (ref.locate(run, run.cycles // 3), A0, False)]
    one = [bignum(at, target, follow_addr=follow) for at, target, follow in places]
    with _job("bignum", 14, ', "devices": [0, 0]') as (origin, n, p):
        assert n == 7
        two = [origin(at, target, follow_addr=follow) for at, target, follow in places]
    for (at, target, follow), a, b in zip(places, one, two):
        assert without_ms(a) == without_ms(b), at
        check(b, elf, stdin, 14, at, target, "bignum on two members at %s" % (at,), follow_addr=follow)


def test_a_partial_job_is_refused():
    from dvt_circuits_amd import capi

    for first in (0, 1):
        with _job("bignum", 14, first=first, stride=2) as (origin, n, p):
            with pytest.raises(capi.DvtError) as e:
                origin(EXIT, A1)
            assert e.value.code == capi.DVT_ERR_UNSUPPORTED


@pytest.mark.parametrize("extra", ["", ', "keep_phase1": 0'])
def test_the_job_is_left_as_found(extra):
    """the proof of a job that was asked before and after proving equals that of a job that never was"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    places = [((2, 100), A0), (EXIT, A1)]
    proofs = []
    for inspect in (True, False):
        p = _prover(11, extra)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = [p.job_origin(pk, job, at, target) for at, target in places] if inspect else None
        proofs.append(p.prove_job(pk, job))
        if inspect:
            after = [p.job_origin(pk, job, at, target) for at, target in places]
            assert [without_ms(s) for s in before] == [without_ms(s) for s in after]
            assert p.prove_job(pk, job) == proofs[0]
            for (at, target), got in zip(places, before):
                check(got, elf, (), 11, at, target, "commit_only at %s" % (at,))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why


def test_the_times_of_a_call():
    with _job("bignum", 14) as (origin, n, p):
        got = origin(EXIT, A1)
        t = p.job_origin_times()
        print(t, got["summary"])
        assert sorted(t) == ["gather_ms", "host_ms", "reduce_ms"] and all(0 < v < 5000 for v in t.values()), t
        assert abs(sum(t.values()) - got["summary"]["ms"]) < 0.01 * got["summary"]["ms"] + 0.01


def test_cli_check_origin(tmp_path):
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(example, "rb").read())
    run = ref.model_run(elf, (buf,))
    base = [CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path)]
    r = subprocess.run(base + ["--origin", "exit:reg:a1", "--depth", "12", "--follow-addr"], capture_output=True, text=True, timeout=120)
    print(r.stdout[:2000], r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ") and r.stdout.splitlines()[1].startswith("origin: ")
    want = ref.slice_of(run, EXIT, A1, True, 12)
    assert want["nodes"]
    cli_agrees(r.stdout, want, False)
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith("clean: ") and len(plain.stdout.splitlines()) == 1
