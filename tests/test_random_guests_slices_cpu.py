"""CPU tests of the origin slice and the divergence report on seeded random guests (tests/guests_random.py), no GPU.

Origin: the host path (capi.execute_origin) on the pinned cases, at 2^9 and 2^21 cycles per shard, against the rule written over
the model's rows (tests/_origin_ref.slice_of) and the two yardsticks that do not depend on the rule (edges_agree, root_agrees).
Divergence: the host path (capi.execute_diverge) on the guests with the input prologue, run on the pairs of inputs of
gr.INPUT_CASES, against the chain of segments of tests/_diverge_ref.  The two coverage tests compute, from the model's runs
alone, what the lists are there to contain: the instruction kinds, leaves and shapes a slice must reach, the mask bits, diffs,
splits and skips a chain must reach.  Every comparison is of exact integers.

slices_of(), origin_places() and the streams are shared with tests/test_gpu_random_guests.py, which runs the same positions and
targets through the prepared jobs."""
import collections
import functools
import random
import struct

import pytest

from dvt_circuits_amd import capi
from tests import _diverge_ref as dref
from tests import _origin_ref as oref
from tests import _profile_ref, guests
from tests import guests_random as gr
from tests.test_random_guests_cpu import CASE_IDS, LOGS, guest_of, run_of

RA = 1
N_WORDS = 8
INPUT_IDS = [gr.input_case_id(e) for e in gr.INPUT_CASES]
SHIFTS = ("sll", "srl", "sra", "slli", "srli", "srai")


# ---------------------------------------------------------------------------------------------- origin: places and targets
def pool_targets():
    return [capi.origin_reg(name) for name in gr.POOL]


def word_targets(guest, run, n=N_WORDS):
    """the n most stored words of the scratch area (ties: the lower address first); none in the alu profile, which has no stores"""
    stores = collections.Counter(r.maddr & ~3 for sh in run.shards for r in sh["rows"]
                                 if r.ins.kind in ("sb", "sh", "sw") and guest.scratch <= r.maddr < guest.scratch + 4 * gr.SCRATCH_WORDS)
    words = sorted(stores, key=lambda a: (-stores[a], a))[:n]
    assert len(words) == (0 if guest.profile == "alu" else n), (guest.seed, len(words))
    return [capi.origin_word(a) for a in words]


def origin_places(case, log_shard, subset=False):
    """[(name of the position, (shard, row) at this shard size, its global record number, targets)]: the first record of the
    ending, the middle of the random part, the first and the last record of the 2^9 shard that follows the one the random part
    begins in, each with the ten pool registers, ra in the flow cases and the eight most stored scratch words; and the exit
    with the words of the `out` area.  The positions are the same records at every shard size.  subset: five of the registers
    and four of the words (and five of the out words), chosen by the case's seed"""
    guest, run = guest_of(case), run_of(case, log_shard)
    first, end = gr.random_span(guest, run)
    edge = (first // 512 + 1) * 512
    regs, words = pool_targets(), word_targets(guest, run)
    outs = [capi.origin_word(guest.out + 4 * k) for k in range(len(gr.POOL))]
    if subset:
        rng = random.Random(case[0])
        regs, words, outs = rng.sample(regs, 5), rng.sample(words, min(4, len(words))), rng.sample(outs, 5)
    targets = regs + ([capi.origin_reg(RA)] if case[1] == "flow" else []) + words
    records = (("end", end), ("middle", (first + end) // 2), ("shard row 0", edge), ("shard row 511", edge + 511))
    return [(name, oref.locate(run, g), g, targets) for name, g in records] + [("exit", oref.EXIT, run.cycles, outs)]


@functools.lru_cache(maxsize=None)
def state_of(case, log_shard, g):
    return oref.state_at(guest_of(case).elf, (), log_shard, g)


def row_of(run, node):
    return run.shards[node["shard"] - 1]["rows"][node["row"]]


def where_of(case, log_shard, name, at, target, follow):
    what = "register %s" % capi.REG_NAMES[target[1]] if target[0] == oref.REG else "word 0x%08x" % target[1]
    return "seed %d profile %s n %d at 2^%d, position %s %s, %s, follow_addr %s" % (case[0], case[1], case[2], log_shard, name, tuple(at), what, follow)


def first_differing_record(run, got, want):
    """gr.describe of the record of the first node that differs between two slices (a node of its own, or the node whose input
    edges differ); "" when the nodes and edges are equal"""
    for k in range(max(len(got["nodes"]), len(want["nodes"]))):
        a, b = (part[k] if k < len(part) else None for part in (got["nodes"], want["nodes"]))
        if a != b:
            n = b or a
            return "node %d: %s" % (k, gr.describe(run, n["shard"] - 1, n["row"]))
    for k in range(max(len(got["edges"]), len(want["edges"]))):
        a, b = (part[k] if k < len(part) else None for part in (got["edges"], want["edges"]))
        if a != b:
            e = b or a
            if e["from"] == oref.NONE:
                return "the root edge"
            n = want["nodes"][e["from"]]
            return "edge %d out of node %d: %s" % (k, e["from"], gr.describe(run, n["shard"] - 1, n["row"]))
    return ""


def held(got, want, run, where, host):
    """oref.same, with the record of the first differing node in the message"""
    try:
        oref.same(got, want, host=host, where=where)
    except AssertionError as e:
        raise AssertionError("%s: %s\n%s" % (where, first_differing_record(run, got, want), e)) from None


def check_origin(call, case, log_shard, subset=False, device=False):
    """every place, target and follow_addr of a case through call(at, target, follow_addr) -> slice, against the rule and both
    yardsticks; returns (slices, edges checked, roots compared)"""
    run = run_of(case, log_shard)
    slices = edges = roots = 0
    for name, at, g, targets in origin_places(case, log_shard, subset):
        for target in targets:
            for follow in (False, True):
                where = where_of(case, log_shard, name, at, target, follow)
                got = call(at, target, follow)
                want = oref.slice_of(run, at, target, follow)
                held(got, want, run, where, host=not device)
                assert got["summary"]["position"] == g, where
                if device:
                    assert got["summary"]["passes"] == sum(-(-q // 256) for q in want["level_questions"]), where
                edges += oref.edges_agree(got, where)
                roots += oref.root_agrees(got, target, state_of(case, log_shard, g), where)
                slices += 1
    return slices, edges, roots


def host_origin(case, log_shard):
    elf = guest_of(case).elf

    def call(at, target, follow):
        rc, rep, got, err = capi.execute_origin(elf, [], at, target, log_shard=log_shard, follow_addr=follow)
        assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, (case, at, target, err)
        return got
    return call


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_host_origins_are_the_models(case, log_shard):
    slices, edges, roots = check_origin(host_origin(case, log_shard), case, log_shard)
    print(gr.case_id(case), "2^%d" % log_shard, "slices", slices, "edges checked", edges, "roots compared", roots)
    assert slices >= 2 * (4 * (10 if case[1] == "alu" else 18) + 10) and edges > 1000 and roots == slices


def test_a_difference_names_the_record():
    """a changed node is reported with the seed, the profile, the position, the target and the instruction of its record"""
    case = gr.CASES[0]
    run = run_of(case, 9)
    name, at, g, targets = origin_places(case, 9)[0]
    want = oref.slice_of(run, at, targets[0])
    assert len(want["nodes"]) > 3
    bad = dict(want, nodes=[dict(n) for n in want["nodes"]])
    bad["nodes"][2]["rs1"] ^= 1
    where = where_of(case, 9, name, at, targets[0], False)
    with pytest.raises(AssertionError) as e:
        held(bad, want, run, where, host=False)
    n = want["nodes"][2]
    text = str(e.value)
    assert all(s in text for s in ("seed 0 profile mixed", "position end", "register t1", "node 2: " + gr.describe(run, n["shard"] - 1, n["row"]))), text
    held(want, want, run, where, host=False)


# ---------------------------------------------------------------------------------------------- origin: what the list contains
def origin_coverage(case, cov):
    """the counters of the slices of one case at 2^9 from `end`: the ten pool registers and the eight words, follow_addr off and on"""
    guest, run = guest_of(case), run_of(case, 9)
    _, end = gr.random_span(guest, run)
    at = oref.locate(run, end)
    for target in pool_targets() + ([capi.origin_reg(RA)] if case[1] == "flow" else []) + word_targets(guest, run):
        for follow in (False, True):
            s = oref.slice_of(run, at, target, follow)
            edges = s["edges"]
            for n in s["nodes"]:
                r = row_of(run, n)
                m = _profile_ref.mnemonic(r.ins.word)
                ins = edges[n["first_edge"]:n["first_edge"] + n["n_edges"]] if n["n_edges"] else []
                roles = [e["role"] for e in ins]
                expanded = not n["flags"] & oref.UNEXPANDED
                cov[("kind", n["kind"])] += 1
                cov[("op", m)] += 1
                if not expanded:
                    continue
                if m in ("sb", "sh") and [e["value"] for e in ins if e["role"] == oref.MEM] == [r.m_prev]:
                    cov[("sub_store_mem", m)] += 1
                if m in ("lui", "auipc", "jal") and n["n_edges"] == 0 and n["first_edge"] == 0:
                    cov[("no_inputs", m)] += 1
                if m in ("jal", "jalr") and r.ins.rd == RA:
                    cov[("writes_ra", m)] += 1
                op = r.ins.word & 0x7F
                if op == 0x33:
                    # an R-type reads both registers: one edge each, none for x0
                    assert roles == [oref.RS1] * bool(r.ins.rs1) + [oref.RS2] * bool(r.ins.rs2), (case, m, roles)
                    if not r.ins.rs1 or not r.ins.rs2:
                        cov[("x0_source", "rtype")] += 1
                if op == 0x13 and not r.ins.rs1:
                    assert roles == [], (case, m, roles)
                    cov[("x0_source", "itype")] += 1
                if op == 0x03 and follow:
                    assert roles == [oref.ADDR] * bool(r.ins.rs1) + [oref.MEM], (case, m, roles)
                    if not r.ins.rs1:
                        cov[("load_x0_no_addr",)] += 1
            for e in edges:
                if e["flags"] & oref.INITIAL:
                    cov[("leaf", "image" if e["flags"] & oref.IMAGE else "low" if e["role"] == oref.MEM and e["target"] < 2048 else "other")] += 1
            cov[("slices",)] += 1
            cov[("depth_64_unexpanded",)] += s["summary"]["depth"] == 64 and any(n["flags"] & oref.UNEXPANDED and n["depth"] == 64 for n in s["nodes"])
            cov[("four_shards",)] += len({n["shard"] for n in s["nodes"]}) >= 4
            cov[("relinked",)] += s["summary"]["n_edges"] > s["summary"]["n_nodes"] and any(
                e["to"] != oref.NONE and e["to"] < k for k, e in enumerate(edges[1:]))
            cov[("capped",)] += s["summary"]["n_nodes"] == oref.MAX_NODES
    return cov


def origin_required():
    keys = [("kind", k) for k in (oref.OP, oref.LOAD, oref.F_STORE)]
    keys += [("sub_store_mem", "sb"), ("sub_store_mem", "sh"), ("x0_source", "rtype"), ("x0_source", "itype"), ("load_x0_no_addr",)]
    keys += [("op", "mul"), ("op", "mulhu"), ("leaf", "image"), ("leaf", "low"), ("depth_64_unexpanded",), ("four_shards",), ("relinked",)]
    return keys


def test_origin_slices_cover_what_they_are_there_for():
    """over the slices from the first record of the ending (never a register at the exit: the ending's hash overwrites the pool):
    nodes of every kind a random guest has; sb and sh nodes whose MEM edge carries m_prev; nodes without input edges; jal / jalr
    writing ra; the cpu chip's mul and mulhu, a shift, a mulh, a division; x0 as a source, with one edge less; a load from
    x0 + offset without an ADDR edge; image leaves and leaves of low memory nothing wrote; the depth limit; four shards; an
    edge to a node that already exists"""
    cov = collections.Counter()
    for case in gr.CASES:
        before = collections.Counter(cov)
        origin_coverage(case, cov)
        d = cov - before
        print(gr.case_id(case), " ".join("%s=%d" % ("/".join(str(x) for x in k), v) for k, v in sorted(d.items(), key=str) if k[0] != "op"))
    print("ops in slices:", " ".join("%s=%d" % (k[1], v) for k, v in sorted(cov.items(), key=str) if k[0] == "op"))
    lacking = [k for k in origin_required() if not cov[k]]
    assert lacking == [], lacking
    assert sum(cov[("no_inputs", m)] for m in ("lui", "auipc", "jal")) > 0 and sum(cov[("writes_ra", m)] for m in ("jal", "jalr")) > 0
    assert sum(cov[("op", m)] for m in SHIFTS) and cov[("op", "mulh")] + cov[("op", "mulhsu")] and sum(cov[("op", m)] for m in ("div", "divu", "rem", "remu"))
    # the two positions inside a shard lie in the random part or at its end in every case
    for case in gr.CASES:
        first, end = gr.random_span(guest_of(case), run_of(case, 9))
        places = origin_places(case, 9)
        assert first < places[2][2] < end and places[2][1][1] == 0 and places[3][1][1] == 511 and places[3][1][0] == places[2][1][0], (case, first, end)
        assert [g for _, _, g, _ in places[:4]] == [g for _, _, g, _ in origin_places(case, 21)[:4]]


# ---------------------------------------------------------------------------------------------- divergence
@functools.lru_cache(maxsize=None)
def input_guest(case):
    return gr.build(case[0], case[2], case[1], stdin_words=gr.INPUT_WORDS)


@functools.lru_cache(maxsize=None)
def streams_of(entry, log_shard):
    """(stream A, stream B) of the model's runs of an entry's guest on its two inputs"""
    elf = input_guest(entry[0]).elf
    runs = [_profile_ref.model_run(elf, (buf,), log_shard) for buf in gr.inputs_of(entry)]
    assert all(run.halted and run.error == "" and run.exit_code == 0 for run in runs), entry
    return tuple(dref.stream_of(run) for run in runs)


def random_first(entry, log_shard=9):
    """the global number of the first record of the random part (the same in both runs: the prologue is straight)"""
    guest = input_guest(entry[0])
    runs = [_profile_ref.model_run(guest.elf, (buf,), log_shard) for buf in gr.inputs_of(entry)]
    firsts = [gr.random_span(guest, run)[0] for run in runs]
    assert firsts[0] == firsts[1]
    return firsts[0]


def chains_agree(got, want, where):
    assert len(got) == len(want), (where, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        dref.same(g, w, "%s, segment %d" % (where, k))


def host_diverge(entry, log_shard):
    elf = input_guest(entry[0]).elf
    a, b = gr.inputs_of(entry)

    def call(**kw):
        rc, reps, got, err = capi.execute_diverge(elf, a, b, log_shard=log_shard, **kw)
        assert rc == capi.DVT_OK and got["summary"]["launched_pairs"] == 0, (entry, rc, err)
        return got
    return call


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("entry", gr.INPUT_CASES, ids=INPUT_IDS)
def test_host_divergence_is_the_models(entry, log_shard):
    sa, sb = streams_of(entry, log_shard)
    call = host_diverge(entry, log_shard)
    where = "%s at 2^%d" % (gr.input_case_id(entry), log_shard)
    want = dref.chain(sa, sb, 64, keep=16)
    chains_agree(dref.chain(sa, sb, 64, keep=16, call=call), want, where)
    dref.same(call(keep=64), dref.report(sa, sb, keep=64), where + ", keep 64 from the entry")
    limit = random_first(entry) + 100
    cut = dref.report(sa, sb, max_pairs=limit, rejoin=True)
    dref.same(call(max_pairs=limit, rejoin=True), cut, where + ", max_pairs %d" % limit)
    assert cut["summary"]["reason"] in (dref.LIMIT, dref.SPLIT) and cut["summary"]["n_pairs"] <= limit


def test_the_prologue_copies_the_input_and_leaves_the_rest():
    """with stdin_words = 0 the ELF is the one without the parameter; with K words the random part's text is the same, the
    scratch slots hold the input when the random part begins, and only a0, a1, t0 and t3 are written before the pool is loaded"""
    case = gr.CASES[0]
    assert gr.random_guest(case[0], case[2], case[1], stdin_words=0) == guest_of(case).elf
    plain, guest = guest_of(case), input_guest(case)
    assert len(guest.slots) == len(set(guest.slots)) == gr.INPUT_WORDS and plain.slots == () and guest.scratch == plain.scratch
    assert input_guest(case).slots == gr.build(case[0], 50, case[1], stdin_words=gr.INPUT_WORDS).slots     # the slots depend on the seed alone
    assert gr.build(case[0], case[2], case[1], stdin_words=4).slots != gr.build(case[0] + 1, case[2], case[1], stdin_words=4).slots
    entry = next(e for e in gr.INPUT_CASES if e[0] == case)
    buf = gr.inputs_of(entry)[0]
    run = _profile_ref.model_run(guest.elf, (buf,), 21)
    rows = run.shards[0]["rows"]
    first, end = gr.random_span(guest, run)
    p_first, p_end = gr.random_span(plain, run_of(case, 21))
    # the same instructions, but for the pc-relative addresses the prologue moved
    shift = guest.random_pcs[0][0] - plain.random_pcs[0][0]
    assert shift == 4 * (first - p_first) > 0 and guest.random_pcs[0][1] - plain.random_pcs[0][1] == shift
    lo, hi = plain.random_pcs[0]
    assert _text(guest.elf, lo + shift, hi + shift) == _text(plain.elf, lo, hi) and hi - lo > 4 * 1000
    state = oref.state_at(guest.elf, (buf,), 21, first)
    for k, slot in enumerate(guest.slots):
        assert state.mem[guest.scratch + 4 * slot] == int.from_bytes(buf[4 * k:4 * k + 4], "little")
    written = set(capi.REG_NAMES[r.ins.rd] for r in rows[:first])
    assert written <= set(("zero", "s0", "sp", "a0", "a1", "t0", "t3") + gr.POOL), written
    # the hint went to the heap, not into the image: the hinted words are leaves
    assert all(guests.HEAP + 4 * k not in run.image_mem for k in range(gr.INPUT_WORDS))


def test_the_tool_passes_the_input_words_on(tmp_path, capsys):
    from tools import random_guest

    path = tmp_path / "g.elf"
    assert random_guest.main(["12", "mixed", "300", "-o", str(path), "--log-shard", "9", "--first-diff", "--stdin-words", "16", "--stdin-seed", "3"]) == 0
    assert path.read_bytes() == gr.random_guest(12, 300, "mixed", stdin_words=16) != gr.random_guest(12, 300, "mixed")
    run = _profile_ref.model_run(path.read_bytes(), (gr.input_of(3, 16),), 9)
    out = capsys.readouterr().out
    assert "%d cycles in %d shards of 2^9" % (run.cycles, len(run.shards)) in out and "host against model: equal, cell by cell" in out


def _text(elf, lo, hi):
    """the bytes of the addresses lo .. hi of an ELF's loaded segments"""
    phoff, = struct.unpack_from("<I", elf, 28)
    phentsize, phnum = struct.unpack_from("<HH", elf, 42)
    for k in range(phnum):
        p_type, off, vaddr, _, filesz = struct.unpack_from("<5I", elf, phoff + k * phentsize)
        if p_type == 1 and vaddr <= lo and hi <= vaddr + filesz:
            return elf[off + lo - vaddr:off + hi - vaddr]
    raise AssertionError("no segment holds 0x%x .. 0x%x" % (lo, hi))


def diverge_counters(entry):
    """the counters of one entry's chain at 2^9, from the model's runs alone"""
    guest = input_guest(entry[0])
    sa, sb = streams_of(entry, 9)
    segs = dref.chain(sa, sb, 64, keep=1 << 30)
    c = collections.Counter(segments=len(segs), cycles_a=len(sa), cycles_b=len(sb))
    uneven = False
    for seg in segs:
        s = seg["summary"]
        c["data"] += s["n_data"]
        c["load_diffs"] += s["n_load_diffs"]
        c["store_diffs"] += s["n_store_diffs"]
        c["mask"] |= s["mask"]
        for e in seg["first"]:
            if uneven and e["shard_a"] != e["shard_b"]:
                c["shards_apart"] += 1
            if not guest.in_random_part(e["pc"]):
                continue
            c["random_data"] += 1
            c["random_mask"] |= e["mask"]
            row = sa.rows[sa.global_of((e["shard_a"], e["row_a"]))]
            assert row.ins.pc == e["pc"]
            if e["mask"] & dref.RD and row.ins.rd:
                c["random_rd_regs"] |= 1 << row.ins.rd
            if e["dir"] == 1 and e["mask"] & dref.MEM:
                c["random_load_diffs"] += 1
            if e["dir"] == 2 and e["after_a"] != e["after_b"]:
                c["random_store_diffs"] += 1
                c["random_sub_store_diffs"] += row.ins.kind in ("sb", "sh")
        if s["reason"] == dref.SPLIT:
            c["splits"] += 1
            if s["rejoin_skip_a"] == dref.NO_REJOIN:
                c["not_rejoined"] += 1
                continue
            c["skip_a_only"] += s["rejoin_skip_a"] > 0 == s["rejoin_skip_b"]
            c["skip_b_only"] += s["rejoin_skip_b"] > 0 == s["rejoin_skip_a"]
            c["skips"] = (c["skips"] or ()) + ((s["rejoin_skip_a"], s["rejoin_skip_b"]),)
            uneven = uneven or s["rejoin_skip_a"] != s["rejoin_skip_b"]
    c["reason"] = segs[-1]["summary"]["reason"]
    return c


def test_input_cases_cover_what_they_are_there_for():
    """from the model's runs alone, over the chains of the pinned entries at 2^9: every mask bit, a load diff, a store diff and a
    sub-word store diff on pairs inside the random part; ten splits, every one rejoined, with skips on one side only, both
    ways; a chain of six segments; a quiet pair of inputs; two runs of different lengths; and, behind a rejoin with unequal
    skips, data pairs whose two records lie in different shards"""
    assert 6 <= len(gr.INPUT_CASES) <= 10 and set(e[0][1] for e in gr.INPUT_CASES) == set(gr.PROFILES) and set(e[1] for e in gr.INPUT_CASES) == {"bit", "other"}
    assert all(e[0] in gr.CASES for e in gr.INPUT_CASES) and (2, "mixed", 6000) in [e[0] for e in gr.INPUT_CASES]
    every = []
    for entry in gr.INPUT_CASES:
        a, b = gr.inputs_of(entry)
        wa, wb = ([int.from_bytes(buf[k:k + 4], "little") for k in range(0, 4 * gr.INPUT_WORDS, 4)] for buf in (a, b))
        if entry[1] == "bit":
            assert sorted(bin(x ^ y).count("1") for x, y in zip(wa, wb)) == [0] * (gr.INPUT_WORDS - 1) + [1]
        else:
            assert all(x != y for x, y in zip(wa, wb))
        c = diverge_counters(entry)
        every.append(c)
        print(gr.input_case_id(entry), " ".join("%s=%s" % (k, ("0x%x" % v if "regs" in k else v)) for k, v in sorted(c.items())))
        assert len(streams_of(entry, 9)[0].sizes) >= 13, entry
    total = lambda k: sum(c[k] for c in every)
    mask = 0
    for c in every:
        mask |= c["random_mask"]
    assert mask == 15, mask
    assert total("random_load_diffs") and total("random_store_diffs") and total("random_sub_store_diffs")
    assert total("splits") >= 10 and total("not_rejoined") == 0
    assert total("skip_a_only") and total("skip_b_only")
    assert max(c["segments"] for c in every) >= 6
    assert any(c["splits"] == 0 and c["data"] < 16 and c["reason"] == dref.END_BOTH for c in every)
    assert any(c["cycles_a"] != c["cycles_b"] for c in every)
    assert total("shards_apart")
    regs = 0
    for c in every:
        regs |= c["random_rd_regs"]
    assert bin(regs).count("1") >= 10, hex(regs)
