"""GPU tests of the uses slice of a prepared job (uses_next_kernel, uses_count_kernel, uses_scan_kernel, uses_emit_kernel and
origin_gather_kernel through dvt_rv32_job_uses / Prover.job_uses).

Every case holds the device's answer against the rule written over the independent model's rows (tests/_uses_ref.uses_of), the
three yardsticks that do not depend on the rule (inverse_of_origin, counts_agree, values_agree) and the host path
(capi.execute_uses at the same shard size), dict for dict except ms and passes.  summary.passes is the sum over the reference's
levels of ceil(definitions / 256).  Every comparison is of exact integers, and every property of a shape is asserted on the
reference's answer inside the test (tests/_uses_ref.shape_of).
Shapes: bignum(40) at 2^14 cycles per shard is seven shards, four spans of 4096 records in each full one and a ragged last
shard of 4160 records; at 2^10 every shard is smaller than a span."""
import contextlib
import functools

import pytest

from tests import _uses_ref as ref
from tests import guests
from tests._watch_ref import _calls
from tests.test_watch_host import hammer_slot, rows_of, watched

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
EXIT = ref.EXIT
A0, S0, A3 = (ref.REG, 10), (ref.REG, 8), (ref.REG, 13)


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


@contextlib.contextmanager
def _job_of(elf, stdin, log_shard, extra="", first=0, stride=1):
    """(uses(at, target, **kw) on the prepared job of the guest, its number of shards, the prover)"""
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, list(stdin), first=first, stride=stride)
    uses = lambda at, target, **kw: p.job_uses(pk, job, at, target, **kw)
    uses.p, uses.pk, uses.job = p, pk, job
    try:
        yield uses, p.job_shards(job), p
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
    """one device answer against the rule, the three yardsticks and the host path; returns (the rule's answer, its shape)"""
    from dvt_circuits_amd import capi

    run = ref.model_run(elf, stdin, log_shard)
    follow = kw.get("follow_addr", False)
    want = ref.uses_of(run, at, target, follow, kw.get("depth", ref.MAX_DEPTH), kw.get("fan", ref.DEFAULT_FAN), kw.get("nodes", ref.MAX_NODES),
                       kw.get("defs", ref.MAX_DEFS), kw.get("edges", ref.MAX_EDGES))
    ref.check(got, run, want, follow, where=where)
    assert got["summary"]["passes"] == sum(-(-q // 256) for q in want["level_defs"]), where
    rc, rep, host, err = capi.execute_uses(elf, list(stdin), at, target, log_shard=log_shard, **kw)
    assert rc == 0 and without_ms(host) == without_ms(got, passes=0), (where, err)
    return want, ref.shape_of(want, run)


# ---------------------------------------------------------------- bignum(40) at 2^14: spans, shard edges, ranks, chunks
@pytest.fixture(scope="module")
def bignum():
    with _job("bignum", 14) as (uses, n, p):
        assert n == 7
        yield uses


@pytest.mark.parametrize("at", [(2, 4095), (2, 4096), (3, 0), (7, 4159), EXIT])
def test_bignum_roots_at_span_and_shard_edges(bignum, at):
    run = run_of("bignum", 14)
    assert run.cycles == 102464 and len(run.shards[-1]["rows"]) == 4160
    elf, stdin = watched("bignum")
    seen = set()
    for target, fan, follow in ((S0, 1, False), (S0, 16, False), (A3, 1, False), (A3, 16, False), ((ref.REG, 2), 16, True), (A0, 8, False)):
        where = "bignum %s at %s fan %d follow %s" % (target, at, fan, follow)
        got = bignum(at, target, fan=fan, follow_addr=follow)
        want, shape = check(got, elf, stdin, 14, at, target, where, fan=fan, follow_addr=follow)
        seen |= shape
    print(at, sorted(seen))
    if at in ((7, 4159), EXIT):
        assert {"dead", "live_at_exit"} <= seen      # nothing reads them any more
    else:
        # a window [F, N] across a span edge and one across a shard edge; the kept uses of one definition in two spans (the
        # emit ranks carried across spans) and in two shards; a next writer that is a use; more uses than fan
        assert {"window_crosses_span", "window_crosses_shard", "kept_in_two_spans", "kept_in_two_shards", "next_is_use", "truncated", "cut"} <= seen, seen


def test_bignum_a_level_of_two_chunks(bignum):
    elf, stdin = watched("bignum")
    at = (6, 11998)
    got = bignum(at, S0, fan=16, follow_addr=True)
    want, shape = check(got, elf, stdin, 14, at, S0, "bignum s0 at (6, 11998)", fan=16, follow_addr=True)
    s = want["summary"]
    print(s, "widest level", max(want["level_defs"]))
    assert "wide_level" in shape and max(want["level_defs"]) > 256 and s["passes"] > s["levels"] == got["summary"]["levels"]
    assert got["summary"]["passes"] == s["passes"] and s["n_nodes"] == 1024 and s["cut"] > 0
    assert all(e["to"] == ref.NONE and e["dst_shard"] for e in want["edges"] if e["flags"] & ref.CUT)


def test_bignum_small_shards():
    """2^10: every shard is smaller than a span, and the slice spans at least five shards"""
    run = run_of("bignum", 10)
    elf, stdin = watched("bignum")
    assert len(run.shards) == 101 and all(len(sh["rows"]) <= 1024 for sh in run.shards)
    with _job("bignum", 10) as (uses, n, p):
        assert n == 101
        for at, target, fan in (((1, 50), S0, 8), (ref.locate(run, run.cycles // 2), S0, 16), ((1, 0), (ref.REG, 2), 1)):
            want, shape = check(uses(at, target, fan=fan), elf, stdin, 10, at, target, "bignum 2^10 %s at %s" % (target, at), fan=fan)
            if fan > 1:
                assert len({n["shard"] for n in want["nodes"]}) >= 5 and "window_crosses_shard" in shape, (at, shape)
        # store -> load -> op -> store, the store in shard 3 and the rest in shard 4 (hammer's loaded value is dead)
        at, target = (2, 990), (ref.REG, 6)
        want, shape = check(uses(at, target, depth=8), elf, stdin, 10, at, target, "bignum 2^10 store -> load -> op -> store", depth=8)
        chain = ref.store_load_op_store(want)
        assert chain is not None and want["nodes"][chain[0]]["shard"] < want["nodes"][chain[1]]["shard"] == want["nodes"][chain[3]]["shard"]


def test_caps_and_depth_zero(bignum):
    elf, stdin = watched("bignum")
    at = (3, 0)
    want, shape = check(bignum(at, A3, nodes=40), elf, stdin, 14, at, A3, "40 nodes", nodes=40)
    cut = [e for e in want["edges"] if e["flags"] & ref.CUT]
    assert cut and all(e["to"] == ref.NONE and e["dst_shard"] >= 3 for e in cut) and want["summary"]["n_nodes"] == 40
    want, shape = check(bignum(at, A3, defs=30), elf, stdin, 14, at, A3, "30 definitions", defs=30)
    assert want["summary"]["n_defs"] <= 30 and want["summary"]["unexpanded"] > 0
    want, shape = check(bignum(at, A3, edges=64), elf, stdin, 14, at, A3, "64 edges", edges=64)
    assert want["summary"]["n_edges"] <= 64 and want["summary"]["unexpanded"] > 0
    want, shape = check(bignum(at, A3, depth=0), elf, stdin, 14, at, A3, "depth 0", depth=0)
    assert want["summary"]["n_defs"] == 1 and want["nodes"] and all(n["flags"] == ref.UNEXPANDED and n["depth"] == 1 for n in want["nodes"])
    want, shape = check(bignum(at, A3, nodes=0), elf, stdin, 14, at, A3, "no nodes", nodes=0)
    assert want["nodes"] == [] and want["edges"] and all(e["flags"] == ref.CUT for e in want["edges"])


# ---------------------------------------------------------------- words: stores, sub-word stores, calls
def test_hammer_chains_across_shard_edges():
    run = run_of("hammer", 10)
    elf, stdin = watched("hammer")
    slot = hammer_slot(run)
    stores = [(s, i, r) for s, i, r in rows_of(run) if r.ins.kind == "sw" and r.maddr & ~3 == slot]
    s, i, r = next(x for x in stores if x[0] == 1 and x[1] > 900)      # late in shard 1
    with _job("hammer", 10) as (uses, n, p):
        assert n == len(run.shards) == 23
        # the register the store writes out, from the record that made it: op -> store -> load, and op -> op across the shard edge
        at, target = (s, i - 1), (ref.REG, r.ins.rs2)
        want, shape = check(uses(at, target), elf, stdin, 10, at, target, "hammer's stored register")
        kinds = {n["kind"] for n in want["nodes"]}
        assert {ref.OP, ref.F_STORE, ref.LOAD} <= kinds and len({n["shard"] for n in want["nodes"]}) >= 2, (kinds, shape)
        store = next(k for k, n in enumerate(want["nodes"]) if n["kind"] == ref.F_STORE)
        word = next(d for d in want["defs"] if d["node"] == store)
        assert (word["what"], word["target"], word["n_uses"]) == (ref.WORD, slot, 1)
        assert want["nodes"][want["edges"][word["first_edge"]]["to"]]["kind"] == ref.LOAD
        # the slot itself, with the address register followed
        for follow in (False, True):
            check(uses((s, i + 1), (ref.WORD, slot), follow_addr=follow), elf, stdin, 10, (s, i + 1), (ref.WORD, slot), "hammer's slot", follow_addr=follow)


def test_sub_word_stores_use_and_end_their_word():
    run = run_of("sub_stores", 10)
    elf = watched("sub_stores")[0]
    subs = [(s, i, r) for s, i, r in rows_of(run) if r.ins.kind in ("sb", "sh")]
    assert len(subs) == 7
    with _job("sub_stores", 10) as (uses, n, p):
        for s, i, r in subs:
            target = (ref.WORD, r.maddr & ~3)
            want, shape = check(uses((1, 0), target), elf, (), 10, (1, 0), target, "sub_stores before %d:%d" % (s, i))
            root, first = want["defs"][0], want["nodes"][0]
            assert (root["next_shard"], root["next_row"]) == (s, i) == (first["shard"], first["row"]) and "next_is_use" in shape
            assert first["kind"] == ref.F_STORE and want["edges"][0]["role"] == ref.MEM and root["value"] == r.m_prev == first["before"]


def test_calls_read_words_and_define_words_without_values():
    run = run_of("u256_ops", 10)
    elf, stdin = watched("u256_ops")
    calls = [(sh["index"], i, c) for sh in run.shards for i, c in sorted(_calls(sh).items())]
    s, i, c = calls[0]
    read = [a for a, rd, wr in c if rd][0]
    with _job("u256_ops", 10) as (uses, n, p):
        assert n == len(run.shards) > 1
        at, target = (s, i), (ref.WORD, read)
        want, shape = check(uses(at, target), elf, stdin, 10, at, target, "a word a call reads")
        call = want["nodes"][0]
        assert call["kind"] == ref.CALL and (call["shard"], call["row"]) == (s, i) and want["edges"][0]["role"] == ref.MEM
        assert want["defs"][0]["flags"] & ref.NO_VALUE      # the root's first use is a call's: the records do not hold the word
        written = [d for d in want["defs"] if d["node"] == 0 and d["what"] == ref.WORD]
        assert len(written) == sum(1 for _, _, wr in c if wr) >= 8 and all(d["flags"] & ref.NO_VALUE for d in written)
        assert "no_value_used" in shape and any(want["nodes"][want["edges"][d["first_edge"]]["to"]]["kind"] == ref.LOAD for d in written if d["n_edges"])
        check(uses(at, target, follow_addr=True, fan=16), elf, stdin, 10, at, target, "with addresses", follow_addr=True, fan=16)


# ---------------------------------------------------------------- handles and jobs
def test_two_members_give_the_one_device_answer(bignum):
    elf, stdin = watched("bignum")
    places = [((2, 4095), S0, 16, False), ((3, 0), A3, 8, True), ((6, 11998), S0, 16, True), (EXIT, A0, 8, False)]
    one = [bignum(at, target, fan=fan, follow_addr=follow) for at, target, fan, follow in places]
    with _job("bignum", 14, ', "devices": [0, 0]') as (uses, n, p):
        assert n == 7
        two = [uses(at, target, fan=fan, follow_addr=follow) for at, target, fan, follow in places]
    for (at, target, fan, follow), a, b in zip(places, one, two):
        assert without_ms(a) == without_ms(b), at
        check(b, elf, stdin, 14, at, target, "bignum on two members at %s" % (at,), fan=fan, follow_addr=follow)


def test_a_partial_job_is_refused():
    from dvt_circuits_amd import capi

    for first in (0, 1):
        with _job("bignum", 14, first=first, stride=2) as (uses, n, p):
            with pytest.raises(capi.DvtError) as e:
                uses((1, 0), S0)
            assert e.value.code == capi.DVT_ERR_UNSUPPORTED


def test_the_job_is_left_as_found():
    """the proof of a job that was asked before and after proving equals that of a job that never was"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    places = [((1, 0), (ref.REG, 2)), ((2, 100), A0), (EXIT, A0)]
    proofs = []
    for inspect in (True, False):
        p = _prover(11)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = [p.job_uses(pk, job, at, target, follow_addr=True) for at, target in places] if inspect else None
        proofs.append(p.prove_job(pk, job))
        if inspect:
            after = [p.job_uses(pk, job, at, target, follow_addr=True) for at, target in places]
            assert [without_ms(s) for s in before] == [without_ms(s) for s in after]
            assert p.prove_job(pk, job) == proofs[0]
            for (at, target), got in zip(places, before):
                check(got, elf, (), 11, at, target, "commit_only at %s" % (at,), follow_addr=True)
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why


def test_the_times_of_a_call(bignum):
    got = bignum((3, 0), A3)
    t = bignum.p.job_uses_times()
    print(t, got["summary"])
    assert sorted(t) == ["count_ms", "emit_ms", "gather_ms", "host_ms", "next_ms"] and all(v >= 0 for v in t.values()), t
    # host_ms is the call's wall clock less the four others, so the five sum to it; summary.ms is that clock as a float32
    # (24 bits: a relative error of at most 2^-24), and the sum of five doubles adds nothing near that
    assert sum(t.values()) <= got["summary"]["ms"] * (1 + 2.0 ** -23) and t["next_ms"] > 0 and t["count_ms"] > 0 and t["host_ms"] > 0


def test_against_origin_on_the_same_job(bignum):
    """the root writer job_origin finds for (consumer position, target) is the definition's node"""
    p, pk, job = bignum.p, bignum.pk, bignum.job
    checked = 0
    for at, target in (((2, 4095), S0), ((3, 0), A3), ((2, 4096), A3)):
        got = bignum(at, target)
        edges = [e for e in got["edges"] if got["defs"][e["def"]]["node"] != ref.NONE][:3]
        assert edges, (at, target)
        for e in edges:
            d = got["defs"][e["def"]]
            node = got["nodes"][d["node"]]
            back = p.job_origin(pk, job, (e["dst_shard"], e["dst_row"]), (d["what"], d["target"]), depth=0)
            root = back["edges"][0]
            assert (root["src_shard"], root["src_row"]) == (node["shard"], node["row"]), (at, target, e, d, root)
            checked += 1
    assert checked == 9
