"""CPU tests on seeded random guests (tests/guests_random.py), no GPU: the product's executor, host trace expansion and record
reports against the oracle's independent model (oracle/rv32_model.py) on the pinned cases, at 2^21 and 2^9 cycles per shard;
the model's own traces through the generated constraint checker; and the conditions that keep the pinned list from silently
being easy, computed from the model's runs alone.  Every comparison is of exact integers."""
import collections
import hashlib
import struct

import numpy as np
import pytest

from dvt_circuits_amd import capi
from oracle import rv32_model
from tests import _calltree_ref, _memory_ref, _orc, _profile_ref, _snapshot_ref, _watch_ref
from tests import guests_random as gr

LOGS = (21, 9)
CASE_IDS = [gr.case_id(c) for c in gr.CASES]
FLOW = [c for c in gr.CASES if c[1] == "flow"]


def guest_of(case):
    return _guest(*case)


_guests = {}


def _guest(seed, profile, n):
    if (seed, profile, n) not in _guests:
        _guests[(seed, profile, n)] = gr.build(seed, n, profile)
    return _guests[(seed, profile, n)]


def run_of(case, log_shard):
    """the model's run of a case, made once per process (shared with the report references)"""
    return _profile_ref.model_run(guest_of(case).elf, (), log_shard)


def flow_queries(guest, run):
    """one query on a scratch word (the most stored one), and the stores of the whole scratch area"""
    stores = collections.Counter(r.maddr & ~3 for sh in run.shards for r in sh["rows"]
                                 if r.ins.kind in _watch_ref.STORES and guest.scratch <= r.maddr < guest.scratch + 4 * gr.SCRATCH_WORDS)
    word = stores.most_common(1)[0][0]
    return [capi.watch_mem(word), capi.watch_mem(guest.scratch, guest.scratch + 4 * gr.SCRATCH_WORDS, flags=capi.DVT_WATCH_STORE)]


def flow_positions(guest, run):
    """a position in the middle of the random part and the last cycle"""
    first, end = gr.random_span(guest, run)
    return [_snapshot_ref.locate(run, (first + end) // 2), _snapshot_ref.locate(run, run.cycles - 1)]


def test_a_seed_gives_the_same_program_every_time():
    for case in (gr.CASES[0], FLOW[0]):
        assert gr.random_guest(case[0], case[2], case[1]) == gr.random_guest(case[0], case[2], case[1]) == guest_of(case).elf
    assert gr.random_guest(0) != gr.random_guest(1) and gr.random_guest(0, profile="mem") != gr.random_guest(0)
    # pinned: the program of a seed is the same on every machine
    assert hashlib.sha256(gr.random_guest(0, 50, "mixed")).hexdigest()[:16] == PINNED_SHA_OF_SEED_0


PINNED_SHA_OF_SEED_0 = "0744c4e63743667e"


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_execution_and_traces_equal_the_model(case, log_shard):
    elf = guest_of(case).elf
    run = run_of(case, log_shard)
    rc, rep, pv, out, err = capi.execute_io(elf, [])
    assert rc == 0 and run.error == "" and run.halted, (case, err, run.error)
    assert rep["cycles"] == run.cycles and rep["exit_code"] == run.exit_code == 0, case
    assert pv == run.public_values and out == run.stdout and len(out) == 4 * (gr.SCRATCH_WORDS + len(gr.POOL)), case
    dg = hashlib.sha256(pv).digest()
    assert [run.committed.get(k) for k in range(8)] == list(struct.unpack("<8I", dg))
    n = len(run.shards)
    for pos in range(n):
        host, hpubs, hn = capi.rv32_debug_traces(elf, [], log_shard, pos)
        model, mpubs = rv32_model.traces(run, pos)
        assert hn == n and (hpubs == mpubs).all(), (case, log_shard, pos)
        assert [(c["chip_id"], c["log_n"]) for c in host] == [(c["chip_id"], c["log_n"]) for c in model], (case, log_shard, pos)
        for h, m in zip(host, model):
            for part in ("main", "prep"):
                why = gr.first_difference(case, log_shard, run, pos, h, m, part, who="the host expansion")
                assert why is None, why


@pytest.mark.parametrize("case", gr.AIR_CASES, ids=[gr.case_id(c) for c in gr.AIR_CASES])
def test_model_traces_satisfy_the_air(case):
    """the yardstick is checked too: the model's matrices of a third of the cases satisfy every generated constraint and balance
    the LogUp multiset with the verifier-side public-value tuples (at 2^9: every shard boundary is in it)"""
    air = _orc.air("rv32")
    run = run_of(case, 9)
    groups = []
    for pos in range(len(run.shards)):
        chips, pubs = rv32_model.traces(run, pos)
        for ch in chips:
            bad, bc, br = air.check_constraints(ch["chip_id"], ch["main"], ch["prep"], pubs)
            assert bad == 0, (case, pos, ch["chip_id"], bc, br, gr.describe(run, pos, br))
        groups.append((chips, pubs))
    dg = hashlib.sha256(run.public_values).digest()
    extra = [(5, [0x10, 0, 0, 0, k, 0, 0, 0] + list(dg[4 * k:4 * k + 4]) + [0, 0], -1, 1) for k in range(8)]
    assert air.logup_unbalanced(groups, extra=extra)[0] == 0, case


@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_host_reports_are_the_models(case):
    guest = guest_of(case)
    elf, where = guest.elf, gr.case_id(case)
    run = run_of(case, 21)
    entry = struct.unpack_from("<I", elf, 24)[0]
    rc, rep, prof, err = capi.execute_profile(elf)
    assert rc == 0 and rep["halted"], err
    _profile_ref.same_tables(prof, _profile_ref.tally(run), where)
    _profile_ref.flow_law(prof, entry, run.shards[-1]["rows"][-1].ins.pc)
    rc, rep, mem, err = capi.execute_memory(elf, [])
    assert rc == 0, err
    _memory_ref.same_report(mem, _memory_ref.report(run), where)
    _memory_ref.laws(mem)
    rc, rep, tree, err = capi.execute_calltree(elf)
    assert rc == 0, err
    _calltree_ref.same_tree(tree, _calltree_ref.tree(run), where)
    _calltree_ref.sum_laws(tree, entry)


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", FLOW, ids=[gr.case_id(c) for c in FLOW])
def test_host_watch_and_snapshot_are_the_models(case, log_shard):
    guest = guest_of(case)
    elf, where = guest.elf, "%s at 2^%d" % (gr.case_id(case), log_shard)
    run = run_of(case, log_shard)
    queries = flow_queries(guest, run)
    want = _watch_ref.search(run, queries)
    assert all(w["total"] for w in want), where
    rc, rep, found, err = capi.execute_watch(elf, [], queries, keep=16, log_shard=log_shard)
    assert rc == 0, err
    _watch_ref.same(found, want, 16, where)
    ranges = [(guest.scratch, guest.scratch + 4 * (gr.SCRATCH_WORDS + len(gr.POOL)))]
    for at in flow_positions(guest, run):
        rc, rep, snap, err = capi.execute_snapshot(elf, [], at, ranges, frames=64, log_shard=log_shard)
        assert rc == 0, err
        want = _snapshot_ref.take(run, at, ranges, 64)
        _snapshot_ref.same(snap, want, "%s at %s" % (where, at))
        _snapshot_ref.agrees(snap, _snapshot_ref.state_at(elf, (), log_shard, want["summary"]["position"]), run, where)


def test_cases_cover_what_they_are_there_for():
    """from the model's runs alone, over the whole list: every mnemonic at least 20 times in the random part; comparisons
    decided by byte 3, 2, 1, 0 and equal; every branch both ways; the carry shapes of ADD and SUB; the MUL / MULHU operand
    shapes; every sub-word offset and both signs; x0 as rd and as rs1; and at 2^9 a shard boundary inside every random part"""
    assert set(c[1] for c in gr.CASES) == set(gr.PROFILES) and 10 <= len(gr.CASES) <= 14
    assert set(gr.PROVE_CASES) <= set(gr.CASES) and sorted(c[1] for c in gr.PROVE_CASES) == sorted(gr.PROFILES)
    cov = collections.Counter()
    long_cases = 0
    for case in gr.CASES:
        guest, run = guest_of(case), run_of(case, 9)
        gr.coverage(guest, run, cov)
        first, end = gr.random_span(guest, run)
        # a boundary of 2^9 inside the random part, 13 or more shards, the last one partial
        assert first // 512 < (end - 1) // 512, (case, first, end)
        assert len(run.shards) >= 13 and 0 < len(run.shards[-1]["rows"]) < 512, (case, len(run.shards), len(run.shards[-1]["rows"]))
        # at 2^21 one shard of two K0 workgroups of 4096 rows, the second ragged
        assert 4096 < run.cycles < 3 * 4096 and run.cycles % 4096, (case, run.cycles)
        long_cases += first < 4096 < end - 1000 and case[1] != "flow"
    assert long_cases >= 1, "no case whose random part reaches into the second K0 workgroup"
    assert gr.missing(cov) == [], gr.missing(cov)
    # the flow cases call through both `jal ra` and the jump table, some frames deep
    for case in FLOW:
        run = run_of(case, 21)
        ops = collections.Counter(_profile_ref.mnemonic(r.ins.word) for sh in run.shards for r in sh["rows"] if guest_of(case).in_random_part(r.ins.pc))
        assert ops["jalr"] >= 20 and _calltree_ref.tree(run)["max_depth"] >= 4, (case, ops["jalr"])
    # SHORT, the byte-parity case, is several shards at 2^9 too
    short = _profile_ref.model_run(guest_of(gr.SHORT).elf, (), 9)
    assert len(short.shards) >= 10


def test_describe_names_the_instruction():
    case = gr.CASES[0]
    guest, run = guest_of(case), run_of(case, 9)
    first, _ = gr.random_span(guest, run)
    shard, row = _snapshot_ref.locate(run, first)
    text = gr.describe(run, shard - 1, row)
    r = run.shards[shard - 1]["rows"][row]
    assert text.startswith("pc 0x%08x: %s " % (r.ins.pc, _profile_ref.mnemonic(r.ins.word))) and "rd <- 0x%08x" % r.a in text
    # a changed cell is reported with the seed, the chip, the column's name, the row and that instruction
    chips, _ = rv32_model.traces(run, shard - 1)
    cpu = next(c for c in chips if gr.chip_names()[c["chip_id"]][0] == "cpu")
    col = gr.chip_names()[cpu["chip_id"]][1].index("a[1]")
    bad = dict(cpu, main=cpu["main"].copy())
    bad["main"][col, row] += 1
    why = gr.first_difference(case, 9, run, shard - 1, bad, cpu)
    assert gr.first_difference(case, 9, run, shard - 1, cpu, cpu) is None
    assert all(s in why for s in ("seed 0 profile mixed", "shard %d chip cpu column a[1] row %d" % (shard - 1, row), text)), why
    # every mnemonic of the list disassembles to its own name
    seen = set()
    for sh in run.shards:
        for k, r in enumerate(sh["rows"]):
            m = _profile_ref.mnemonic(r.ins.word)
            if m not in seen and m != "ecall":
                seen.add(m)
                assert gr.disassemble(r.ins).split()[0] == m
    assert len(seen) > 40


def test_the_tool_writes_the_guest_and_compares(tmp_path, capsys):
    from tools import random_guest

    path = tmp_path / "g.elf"
    assert random_guest.main(["12", "mixed", "300", "-o", str(path), "--log-shard", "9", "--first-diff"]) == 0
    assert path.read_bytes() == guest_of(gr.SHORT).elf
    out = capsys.readouterr().out
    run = _profile_ref.model_run(guest_of(gr.SHORT).elf, (), 9)
    assert "%d cycles in %d shards of 2^9" % (run.cycles, len(run.shards)) in out and "host against model: equal, cell by cell" in out
    assert all(("\n%s: " % k) in out for k in ("decided", "taken", "carry", "offset", "rd_x0"))
