"""Watchpoints on the host (dvt_execute_watch, no GPU) against the rule written over the independent model's rows and
precompile events (tests/_watch_ref.py): totals and whole hit lists on the stock guests, the merged word of sb / sh, the
precompile hits, a value filter, the history of one word, the tool's spec parser and the CLI.  Every comparison is of exact
integers and whole lists."""
import collections
import functools
import os
import subprocess

import pytest

from dvt_circuits_amd import capi
from tests import _watch_ref as ref
from tests import guests, guests_watch
from tests.test_memory_host import CLI, GOLD, guest
from tools import watch_guest

NAMES = ("arith", "subword", "hint_sum", "bignum", "hammer", "sha256_straddling", "curve_ops", "u256_ops", "sub_stores")
EXTRA = {"sub_stores": lambda: (guests_watch.sub_stores(), ())}
ALL_MEMORY = (0, 0x38000000)
EVERY_DIRECTION = capi.DVT_WATCH_LOAD | capi.DVT_WATCH_STORE | capi.DVT_WATCH_PRE_READ | capi.DVT_WATCH_PRE_WRITE


@functools.lru_cache(maxsize=None)
def watched(name):
    """(elf, stdin buffers) of a guest of tests/test_memory_host.py or of tests/guests_watch.py"""
    return EXTRA[name]() if name in EXTRA else guest(name)


@functools.lru_cache(maxsize=None)
def run_of(name, log_shard=21):
    elf, stdin = watched(name)
    return ref.model_run(elf, stdin, log_shard)


def rows_of(run):
    return [(sh["index"], i, r) for sh in run.shards for i, r in enumerate(sh["rows"])]


def call_words(run):
    """every (word, is read, is write) of every precompile call of the model's run"""
    return [w for sh in run.shards for words in ref._calls(sh).values() for w in words]


def standard_queries(run):
    """Queries that exercise every kind on whatever the guest does, chosen from the model's run (inputs only: which pc is
    hot, which register and which word are written most, where the calls point): the whole text, the hottest pc, the most
    written register with and without a value filter, all of memory in every direction and store by store, the most stored
    word and its neighbours, the range of the calls' arrays read and written, a store of one value, and a windowed pc."""
    rows = rows_of(run)
    pcs = collections.Counter(r.ins.pc for _, _, r in rows)
    hot = pcs.most_common(1)[0][0]
    regs = collections.Counter(r.ins.rd for _, _, r in rows if r.ins.rd)
    reg = regs.most_common(1)[0][0]
    writes = [r.a for _, _, r in rows if r.ins.rd == reg]
    stores = [r for _, _, r in rows if r.ins.kind in ref.STORES]
    word = collections.Counter(r.maddr & ~3 for r in stores).most_common(1)[0][0] if stores else 0x400000
    value = stores[len(stores) // 2].m_val if stores else 0
    calls = call_words(run)
    lo, hi = (min(w[0] for w in calls), max(w[0] for w in calls) + 4) if calls else (word, word + 4)
    mid = rows[len(rows) // 2]
    end = rows[(3 * len(rows)) // 4]
    return [
        capi.watch_pc(run.text_base, run.text_base + 4 * run.n_instr),
        capi.watch_pc(hot),
        capi.watch_reg(reg),
        capi.watch_reg(reg, value=writes[len(writes) // 2], mask=0xFFFF),
        capi.watch_mem(*ALL_MEMORY),
        capi.watch_mem(*ALL_MEMORY, flags=capi.DVT_WATCH_STORE),
        capi.watch_mem(max(word - 8, 0), word + 12, flags=capi.DVT_WATCH_LOAD | capi.DVT_WATCH_STORE),
        capi.watch_mem(lo + 4, lo + 44, flags=capi.DVT_WATCH_PRE_WRITE | capi.DVT_WATCH_STORE),
        capi.watch_mem(lo, hi, flags=capi.DVT_WATCH_PRE_READ),
        capi.watch_mem(*ALL_MEMORY, flags=capi.DVT_WATCH_STORE, value=value),
        capi.watch_pc(run.text_base, run.text_base + 4 * run.n_instr, window=((mid[0], mid[1]), (end[0], end[1]))),
        capi.watch_mem(*ALL_MEMORY, value=value, mask=0xFF),
    ]


def host_watch(name, queries, keep, log_shard=21, **kw):
    elf, stdin = watched(name)
    rc, rep, found, err = capi.execute_watch(elf, list(stdin), queries, keep=keep, log_shard=log_shard, **kw)
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    return found


@pytest.mark.parametrize("name", NAMES)
def test_host_watch_is_the_models(name):
    run = run_of(name)
    queries = standard_queries(run)
    want = ref.search(run, queries)
    print(name, [w["total"] for w in want])
    assert want[0]["total"] == run.cycles and all(w["total"] for w in want[:7])
    for keep in (5, 256, 0):
        ref.same(host_watch(name, queries, keep), want, keep, "%s keep %d" % (name, keep))
    # positions are those of the shard size asked for
    small = run_of(name, 10)
    want = ref.search(small, standard_queries(small))
    assert len(small.shards) > 1 and max(h["shard"] for h in want[0]["hits"]) == len(small.shards)
    ref.same(host_watch(name, standard_queries(small), 7, log_shard=10), want, 7, name + " at 2^10")


def test_subword_stores_merge_into_the_word():
    """sb at every offset 0..3 and sh at 0 and 2 (tests/guests_watch.sub_stores; the stock subword guest has no sb at offset
    2): `after` is the byte or half of rs2 merged into `before`"""
    q = [capi.watch_mem(*ALL_MEMORY, flags=capi.DVT_WATCH_STORE)]
    seen = set()
    for name in ("sub_stores", "subword"):
        run = run_of(name)
        want = ref.search(run, q)
        seen |= {(r.ins.kind, r.maddr & 3) for _, _, r in rows_of(run) if r.ins.kind in ("sb", "sh")}
        merged = [h for h in want[0]["hits"] if h["after"] not in (h["before"], h["rs2"])]
        assert merged, "no store whose word is neither the old word nor rs2"
        ref.same(host_watch(name, q, 256), want, 256)
    assert seen == {("sb", 0), ("sb", 1), ("sb", 2), ("sb", 3), ("sh", 0), ("sh", 2)}
    # spelled out for one of them: sb of 0x98 at offset 2 of 0x99aabbcc
    hit = [h for h in ref.search(run_of("sub_stores"), q)[0]["hits"] if h["before"] == 0x99AABBCC]
    assert [(h["after"], h["rs2"]) for h in hit] == [(0x9998BBCC, 0xFEDCBA98)]


@pytest.mark.parametrize("name", ["sha256_straddling", "curve_ops", "u256_ops"])
def test_precompile_hits_carry_no_value(name):
    run = run_of(name)
    calls = call_words(run)
    lo, hi = min(w[0] for w in calls), max(w[0] for w in calls) + 4
    pre = capi.DVT_WATCH_PRE_READ | capi.DVT_WATCH_PRE_WRITE
    q = [capi.watch_mem(lo, hi, flags=pre), capi.watch_mem(lo, hi, flags=capi.DVT_WATCH_PRE_WRITE), capi.watch_mem(lo + 8, lo + 12, flags=pre),
         capi.watch_mem(lo, hi, flags=pre, value=0, mask=0), capi.watch_mem(lo, hi, flags=EVERY_DIRECTION, value=0, mask=0)]
    want = ref.search(run, q)
    n_calls = sum(len(ref._calls(sh)) for sh in run.shards)
    assert want[0]["total"] == n_calls > 0 and 0 < want[1]["total"] <= n_calls and want[2]["total"] > 0
    assert all(h["flags"] & capi.DVT_WATCH_HIT_NO_VALUE and h["before"] == h["after"] == 0 and h["n_words"] >= 1 for w in want[:3] for h in w["hits"])
    assert {h["n_words"] for h in want[2]["hits"]} <= {1, 2} and max(h["n_words"] for h in want[0]["hits"]) > 8
    # a value filter never matches a call (a mask of 0 matches every load and store)
    assert want[3]["total"] == 0
    assert all(h["flags"] in (capi.DVT_WATCH_LOAD, capi.DVT_WATCH_STORE) for h in want[4]["hits"])
    ref.same(host_watch(name, q, 256), want, 256, name)


def test_a_value_filter_finds_the_stores_of_that_value():
    run = run_of("bignum")
    stores = [(s, i, r) for s, i, r in rows_of(run) if r.ins.kind in ref.STORES]
    value = collections.Counter(r.m_val for _, _, r in stores if r.m_val).most_common(1)[0][0]
    model = [(s, i) for s, i, r in stores if r.m_val == value]
    found = host_watch("bignum", [capi.watch_mem(*ALL_MEMORY, flags=capi.DVT_WATCH_STORE, value=value)], 256)[0]
    assert 0 < found["total"] == len(model) < len(stores)
    assert [(h["shard"], h["row"]) for h in found["last"]] == model[-256:] and all(h["after"] == value for h in found["first"] + found["last"])
    low = [(s, i) for s, i, r in stores if r.m_val & 0xFF == value & 0xFF]
    found = host_watch("bignum", [capi.watch_mem(*ALL_MEMORY, flags=capi.DVT_WATCH_STORE, value=value, mask=0xFF)], 256)[0]
    assert found["total"] == len(low) >= len(model) and [(h["shard"], h["row"]) for h in found["first"]] == low[:256]


def hammer_slot(run):
    hits = collections.Counter(r.maddr & ~3 for _, _, r in rows_of(run) if r.ins.kind in ("lw", "sw"))
    return hits.most_common(1)[0][0]


def test_the_history_of_a_stack_slot_is_the_models():
    """following (prev_shard, prev_clk) backwards from the last access visits the model's accesses of the word in reverse"""
    run = run_of("hammer", 10)
    slot = hammer_slot(run)
    model = [(s, i, r.ins.kind) for s, i, r in rows_of(run) if r.ins.kind in ref.LOADS + ref.STORES and r.maddr & ~3 == slot]
    assert len(model) == 6000 and len({s for s, _, _ in model}) > 10
    calls = []

    def search(queries, keep):
        calls.append(keep)
        return host_watch("hammer", queries, keep, log_shard=10)
    hits, why = watch_guest.history(search, slot + 1)
    assert why == "first touch of the word" and len(calls) <= 6000 // 256 + 2
    assert [(h["shard"], h["row"], "lw" if h["flags"] & capi.DVT_WATCH_LOAD else "sw") for h in hits] == model[::-1]
    # every link of the chain is the position of the hit before it
    for newer, older in zip(hits, hits[1:]):
        assert (newer["prev_shard"], newer["prev_clk"]) == (older["shard"], 4 * older["row"] + 6)
    # "the last writer before row r of shard s": one STORE query with to = (s, r), the last entry of its last list
    s, i, _ = model[4001]
    found = host_watch("hammer", [capi.watch_mem(slot, flags=capi.DVT_WATCH_STORE, window=((0, 0), (s, i)))], 1, log_shard=10)[0]
    before = [(a, b) for a, b, k in model if k == "sw" and (a, b) < (s, i)]
    assert found["total"] == len(before) and (found["last"][-1]["shard"], found["last"][-1]["row"]) == before[-1]


def test_the_history_stops_at_a_precompile_call():
    """u256_ops loads the words a call wrote: such a load points at the call, which is no load or store"""
    run = run_of("u256_ops")
    written = {w[0] for w in call_words(run) if w[2]}
    loads = [(s, i, r) for s, i, r in rows_of(run) if r.ins.kind in ref.LOADS and r.maddr & ~3 in written]
    assert loads
    s, i, r = loads[-1]
    hits, why = watch_guest.history(lambda q, keep: host_watch("u256_ops", q, keep), r.maddr)
    model = [(a, b) for a, b, x in rows_of(run) if x.ins.kind in ref.LOADS + ref.STORES and x.maddr & ~3 == r.maddr & ~3]
    assert hits and "no load or store" in why and [(h["shard"], h["row"]) for h in hits] == model[::-1][:len(hits)]
    call = (hits[-1]["prev_shard"], hits[-1]["prev_clk"] // 4 - 1)
    assert run.shards[call[0] - 1]["rows"][call[1]].ins.kind == "ecall" and "%d:%d" % call in why


SPECS = ["pc:0x2008a0", "pc:0x200000+64", "reg:sp=0x7ff0/0xfff0", "reg:x31", "reg:a0=5", "store:0x400000+64", "mem:0x400000+4=0xdeadbeef",
         "load:0x400004", "pread:0x400000+256", "pwrite:0x400010+8=0x1/0x1"]


@pytest.mark.parametrize("spec", SPECS)
def test_spec_parser_round_trips(spec):
    q = watch_guest.parse_spec(spec)
    assert watch_guest.parse_spec(watch_guest.format_spec(q)) == q
    assert watch_guest.format_spec(watch_guest.parse_spec(watch_guest.format_spec(q))) == watch_guest.format_spec(q)
    window = ((3, 100), (5, 0))
    assert watch_guest.parse_spec(spec, window) == dict(q, from_shard=3, from_row=100, to_shard=5, to_row=0)


def test_specs_are_the_constructors_queries():
    assert watch_guest.parse_spec("pc:0x2008a0") == capi.watch_pc(0x2008A0)
    assert watch_guest.parse_spec("reg:sp=0x7ff0/0xfff0") == capi.watch_reg(2, value=0x7FF0, mask=0xFFF0)
    assert watch_guest.parse_spec("reg:t0") == capi.watch_reg(5)
    assert watch_guest.parse_spec("store:0x400000+64") == capi.watch_mem(0x400000, 0x400040, flags=capi.DVT_WATCH_STORE)
    assert watch_guest.parse_spec("mem:0x400000+4=0xdeadbeef") == capi.watch_mem(0x400000, value=0xDEADBEEF)
    assert watch_guest.parse_position("3:100") == (3, 100) and watch_guest.parse_position("7") == (7, 0)
    for bad in ("reg:x0", "reg:zero", "reg:x32", "jump:0x10", "0x2008a0"):
        with pytest.raises(ValueError):
            watch_guest.parse_spec(bad)


def cli_totals(stdout):
    """the --watch block: {spec: total} and {spec: [hit lines]}"""
    totals, lines, spec = {}, {}, None
    for l in stdout.splitlines():
        if l.startswith("watch "):
            spec, _, t = l[6:].rpartition(": total=")
            totals[spec] = int(t)
            lines[spec] = []
        elif spec and l.startswith("  "):
            lines[spec].append(l.split())
    return totals, lines


def cli_line(h):
    """a hit as the CLI prints it, split at blanks"""
    f = ["%d:%d" % (h["shard"], h["row"]), "pc=0x%08x" % h["pc"], "rd=0x%08x" % h["rd_value"], "rs1=0x%08x" % h["rs1"], "rs2=0x%08x" % h["rs2"]]
    if h["flags"] & (capi.DVT_WATCH_LOAD | capi.DVT_WATCH_STORE):
        f += ["load" if h["flags"] & capi.DVT_WATCH_LOAD else "store", "addr=0x%08x" % h["addr"], "before=0x%08x" % h["before"], "after=0x%08x" % h["after"],
              "prev=%d:%d" % (h["prev_shard"], h["prev_clk"])]
    elif h["flags"] & capi.DVT_WATCH_HIT_NO_VALUE:
        f += ["call", "addr=0x%08x" % h["addr"], "words=%d" % h["n_words"]]
    return f


def cli_case():
    """(elf, the stdin buffer of the golden input, specs) of the CLI tests: hint_sum over the example input"""
    inp = os.path.join(GOLD, "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    elf = guests.hint_sum()
    run = ref.model_run(elf, (buf,))
    hot = collections.Counter(r.ins.pc for _, _, r in rows_of(run)).most_common(1)[0][0]
    specs = ["pc:0x%x" % hot, "reg:t0", "load:0x%x+%d" % (guests.HEAP, len(buf)), "mem:0+0x38000000", "store:0+0x38000000=0x0/0xff"]
    return inp, elf, buf, specs


def test_cli_execute_watch(tmp_path):
    inp, elf, buf, specs = cli_case()
    path = tmp_path / "hint_sum.elf"
    path.write_bytes(elf)
    want = ref.search(ref.model_run(elf, (buf,)), [watch_guest.parse_spec(s) for s in specs])
    base = [CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)]
    r = subprocess.run(base + [x for s in specs for x in ("--watch", s)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    totals, lines = cli_totals(r.stdout)
    assert totals == {s: w["total"] for s, w in zip(specs, want)} and all(w["total"] for w in want[:4])
    for s, w in zip(specs, want):
        assert lines[s] == [cli_line(h) for h in w["hits"][-4:]], s
    # without the flag every byte is as before; a bad spec is refused
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == f"input len: {len(buf) - 8}\n"
    bad = subprocess.run(base + ["--watch", "reg:x0"], capture_output=True, text=True)
    assert bad.returncode != 0 and "watch" in bad.stderr
