"""Snapshots on the host (dvt_execute_snapshot, no GPU) against the rule written over the independent model's rows and
precompile events (tests/_snapshot_ref.take) and against the model stopped at the position (state_at): the nine guests of the
watchpoint tests at 2^12 cycles per shard and five positions each, the NO_VALUE and INITIAL limits, the backtraces of the
call-tree guests, a guest that traps, and the CLI.  Every comparison is of exact integers."""
import functools
import os
import struct
import subprocess

import pytest

from dvt_circuits_amd import capi
from oracle import rv32_model
from tests import _snapshot_ref as ref
from tests import guests, guests_calltree, guests_memory
from tests._watch_ref import _access, _calls
from tests.test_memory_host import CLI, GOLD, HINT
from tests.test_watch_host import NAMES, watched
from tools import snapshot_guest

LOG = 12
PAGE_WORDS = 1024
CLEAN = ("arith", "subword", "hint_sum", "bignum", "hammer", "sub_stores", "curve_ops", "u256_ops")


@functools.lru_cache(maxsize=None)
def run_of(name, log_shard=LOG):
    elf, stdin = watched(name)
    return ref.model_run(elf, stdin, log_shard)


def accessed_words(run):
    """every word a load, a store or a precompile call of the model's run touches"""
    words = set()
    for sh in run.shards:
        for r in sh["rows"]:
            acc = _access(r)
            if acc:
                words.add(acc[1])
        for call in _calls(sh).values():
            words.update(addr for addr, _, _ in call)
    return words


def page_ranges(run):
    """the accessed pages of the guest in address order, cut to 4096 words"""
    pages = sorted(set(w // 4096 for w in accessed_words(run)))[:capi.DVT_SNAP_MAX_WORDS // PAGE_WORDS]
    return [(4096 * p, 4096 * (p + 1)) for p in pages]


def tight_ranges(run):
    """per accessed page the span of its accessed words and two words around it: every accessed word of a guest whose pages
    do not fit, cut to 16 ranges and 4096 words"""
    words, out, total = accessed_words(run), [], 0
    for p in sorted(set(w // 4096 for w in words))[:capi.DVT_SNAP_MAX_RANGES]:
        mine = [w for w in words if w // 4096 == p]
        lo, hi = max(min(mine) - 8, 4096 * p), min(max(mine) + 12, 4096 * (p + 1))
        hi = min(hi, lo + 4 * (capi.DVT_SNAP_MAX_WORDS - total))
        if hi > lo:
            out.append((lo, hi))
            total += (hi - lo) // 4
    return out


def positions(run):
    c = run.cycles
    return [(1, 0), (1, 1), ref.locate(run, c // 3), ref.locate(run, c // 2), ref.EXIT]


def host_snapshot(name, at, ranges, frames=64, log_shard=LOG):
    elf, stdin = watched(name)
    rc, rep, snap, err = capi.execute_snapshot(elf, list(stdin), at, ranges, frames=frames, log_shard=log_shard)
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    return snap


@pytest.mark.parametrize("name", NAMES)
def test_host_snapshot_is_the_models(name):
    run = run_of(name)
    elf, stdin = watched(name)
    assert run.cycles == sum(len(sh["rows"]) for sh in run.shards)
    for ranges in (page_ranges(run), tight_ranges(run)):
        assert ranges and sum((hi - lo) // 4 for lo, hi in ranges) <= capi.DVT_SNAP_MAX_WORDS
        for at in positions(run):
            where = "%s at %s" % (name, at)
            got = host_snapshot(name, at, ranges)
            want = ref.take(run, at, ranges)
            ref.same(got, want, where)
            g = want["summary"]["position"]
            n = ref.agrees(got, ref.state_at(elf, stdin, LOG, g), run, where)
            print(where, "position", g, "words", len(got["words"]), "with a value", n, "no_value", len(ref.no_value(got)),
                  "initial", got["summary"]["initial"], "untouched", got["summary"]["untouched"])
            if name in CLEAN:
                assert ref.no_value(got) == [], where
    # (1, 0): nothing ran; the end: the model's final registers
    first, last = host_snapshot(name, (1, 0), ()), host_snapshot(name, ref.EXIT, ())
    assert all(c["flags"] == (capi.DVT_SNAP_INITIAL if k else 0) and c["value"] == 0 for k, c in enumerate(first["regs"]))
    assert first["summary"]["depth"] == 0 and first["summary"]["pc"] == run.entry
    assert [c["value"] for c in last["regs"]] == run.reg and last["summary"]["pc"] == rv32_model.HALT_PC


def test_the_no_value_words_of_sha256_are_the_references():
    """the schedule and state arrays of sha256_straddling are written by the calls and read by nothing but calls: at the exit
    the words the last call wrote and no load read afterwards carry no value, and name that call"""
    run = run_of("sha256_straddling")
    ranges = tight_ranges(run)
    covered = set(a for lo, hi in ranges for a in range(lo, hi, 4))
    assert accessed_words(run) <= covered
    seen = 0
    for at in positions(run):
        got, want = host_snapshot("sha256_straddling", at, ranges), ref.take(run, at, ranges)
        assert ref.no_value(got) == ref.no_value(want), at
        print(at, "NO_VALUE", len(ref.no_value(got)), "of", len(accessed_words(run)), "accessed words")
        seen = max(seen, len(ref.no_value(got)))
        calls = {(sh["index"], row) for sh in run.shards for row in _calls(sh)}
        for c in got["words"]:
            if c["flags"] & capi.DVT_SNAP_NO_VALUE and not c["flags"] & capi.DVT_SNAP_UNTOUCHED:
                assert (c["shard"], c["row"]) in calls and c["value"] == 0, c
    assert seen > 0


def test_hinted_words_show_their_value_early():
    """hint_sum at (1, 1): nothing has accessed the ten hinted words, the loads that will read them come later: INITIAL with
    the hinted values, which the machine holds only from HINT_READ on"""
    run = run_of("hint_sum")
    hinted = sorted(a for a, v in run.first_val.items() if v)    # (the only words that start with a value and lie outside the image)
    assert len(hinted) == 10 and [run.first_val[a] for a in hinted] == list(struct.unpack("<10I", HINT))
    got = host_snapshot("hint_sum", (1, 1), page_ranges(run))
    cells = {c["addr"]: c for c in got["words"]}
    assert [cells[a]["value"] for a in hinted] == list(struct.unpack("<10I", HINT))
    assert all(cells[a]["flags"] == capi.DVT_SNAP_FROM_AFTER | capi.DVT_SNAP_INITIAL for a in hinted)
    elf, stdin = watched("hint_sum")
    early = ref.state_at(elf, stdin, LOG, 1)
    assert all(early.mem.get(a, 0) == 0 for a in hinted)    # (the model has not hinted them yet: the documented exception)


CALL_GUESTS = {"recurse": guests_calltree.recurse, "tail": guests_calltree.tail, "stray": guests_calltree.stray, "nest": guests_calltree.nest}


@functools.lru_cache(maxsize=None)
def call_guest(name):
    made = CALL_GUESTS[name]()
    return made[0] if isinstance(made, tuple) else made


def deepest(run):
    """the global record number at which the stack of the model's walk is deepest (the first such)"""
    rows = [r for sh in run.shards for r in sh["rows"]]
    depth, best, at = 0, 0, 0
    for g, r in enumerate(rows):
        if g == 0:
            depth = 1
        ev = ref._calltree_ref.event_of(r.ins.word)
        if ev == "call" and r.next_pc in run.text:
            depth += 1
        elif ev == "ret" and depth > 1:
            depth -= 1
        if depth > best:
            best, at = depth, g + 1
    return at, best


@pytest.mark.parametrize("name", sorted(CALL_GUESTS))
@pytest.mark.parametrize("log_shard", (10, 14))
def test_backtraces_are_the_walks(name, log_shard):
    elf = call_guest(name)
    run = ref.model_run(elf, (), log_shard)
    deep, depth = deepest(run)
    c = run.cycles
    for g in sorted({0, 1, 2, c // 4, c // 2, deep - 1, deep, deep + 1, c - 1, c}):
        at = ref.locate(run, g) if g < c else ref.EXIT
        for frames in (8, 512):
            rc, rep, got, err = capi.execute_snapshot(elf, [], at, (), frames=frames, log_shard=log_shard)
            assert rc == 0, err
            want = ref.take(run, at, (), frames)
            ref.same(got, want, "%s at %d frames %d" % (name, g, frames))
            if g == deep:
                assert got["summary"]["depth"] == depth and got["summary"]["n_frames"] == min(frames, depth)
    # every frame's call record is the model's row before the frame opened
    rows = [r for sh in run.shards for r in sh["rows"]]
    got = capi.execute_snapshot(elf, [], ref.locate(run, deep), (), frames=512, log_shard=log_shard)[2]
    assert len(got["frames"]) == depth and got["frames"][-1]["call_pc"] == 0xFFFFFFFF
    for f in got["frames"][:-1]:
        opened = sum(len(sh["rows"]) for sh in run.shards[:f["open_shard"] - 1]) + f["open_row"]
        assert (f["call_pc"], f["ra"], f["fn_pc"]) == (rows[opened - 1].ins.pc, rows[opened - 1].a, rows[opened].ins.pc), f
    if name == "stray":
        assert capi.execute_snapshot(elf, [], ref.EXIT, (), log_shard=log_shard)[2]["summary"]["unmatched_returns"] == 1
    if name == "recurse":
        assert depth > 320


def trapping():
    a = guests_memory.Asm()
    buf = a.dword("buf", [1, 2, 3, 4])
    a.li("s1", buf)
    a.lw("a0", "s1", 0)
    a.sw("a0", "s1", 8)
    a.li("s2", guests.HEAP)
    a.sw("a0", "s2", 4)
    a.lw("a4", "s1", 1)            # misaligned: traps
    a.halt(0)
    return a.elf(), buf


def test_a_trapping_guest_snapshots_at_its_trap():
    """the model keeps no rows of the shard that trapped, but its registers and memory: the post-mortem is compared with them"""
    elf, buf = trapping()
    ranges = [(buf, buf + 16), (guests.HEAP, guests.HEAP + 8)]
    rc, rep, got, err = capi.execute_snapshot(elf, [], capi.SNAP_EXIT, ranges)
    rc0, rep0, _, err0 = capi.execute(elf)
    assert rc == rc0 == capi.DVT_ERR_GUEST and rep == rep0 and err == err0 and not rep["halted"]
    run = rv32_model.Run(elf)
    assert run.error and not run.halted and run.cycles == rep["cycles"] == got["summary"]["position"] == got["summary"]["cycles"]
    assert ref.agrees(got, run, run) == 5    # (all but the heap word nothing touched)
    cells = {c["addr"]: c for c in got["words"]}
    assert cells[buf + 8]["value"] == 1 and cells[buf + 8]["flags"] == capi.DVT_SNAP_FROM_BEFORE | capi.DVT_SNAP_STORE
    assert cells[buf]["flags"] == capi.DVT_SNAP_FROM_BEFORE | capi.DVT_SNAP_LOAD
    assert cells[buf + 4]["flags"] == capi.DVT_SNAP_IMAGE | capi.DVT_SNAP_INITIAL | capi.DVT_SNAP_UNTOUCHED and cells[buf + 4]["value"] == 2
    assert cells[guests.HEAP]["flags"] == capi.DVT_SNAP_NO_VALUE | capi.DVT_SNAP_UNTOUCHED
    assert got["summary"]["depth"] == 1 and got["frames"][0]["call_pc"] == 0xFFFFFFFF
    # the state one record earlier: the store to the heap has not happened
    rc, rep, got, err = capi.execute_snapshot(elf, [], (1, rep["cycles"] - 1), ranges)
    assert rc == capi.DVT_ERR_GUEST
    cells = {c["addr"]: c for c in got["words"]}
    assert cells[guests.HEAP + 4]["flags"] == capi.DVT_SNAP_FROM_AFTER | capi.DVT_SNAP_INITIAL and cells[guests.HEAP + 4]["value"] == 0


def max_cycles_case():
    elf, _ = watched("hammer")
    return elf


def test_max_cycles_cuts_the_snapshot():
    elf = max_cycles_case()
    rc, rep, got, err = capi.execute_snapshot(elf, [], capi.SNAP_EXIT, (), max_cycles=1000, log_shard=8)
    assert rc == capi.DVT_ERR_GUEST and rep["cycles"] == got["summary"]["cycles"] == got["summary"]["position"] == 1000
    state = ref.state_at(elf, (), 8, 1000)
    assert [c["value"] for c in got["regs"]] == state.reg


def cli_block(stdout):
    """the --snapshot block: (dict of the summary line, {register name: value}, [frame lines], {addr: word text})"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("snapshot: "))
    summary = {k: int(v, 0) for k, v in (f.split("=") for f in lines[a].split()[1:])}
    regs, frames, words = {}, [], {}
    for l in lines[a + 1:]:
        f = l.split()
        if f and f[0] == "regs":
            regs.update((kv.split("=")[0], int(kv.split("=")[1], 16)) for kv in f[1:])
        elif f and f[0].startswith("#"):
            frames.append(f)
        elif f and f[0].endswith(":") and f[0].startswith("0x"):
            base = int(f[0][:-1], 16)
            for k, w in enumerate(f[1:]):
                words[base + 4 * k] = w
        else:
            break
    return summary, regs, frames, words


def test_cli_execute_snapshot(tmp_path):
    elf = call_guest("recurse")
    path = tmp_path / "recurse.elf"
    path.write_bytes(elf)
    inp = os.path.join(GOLD, "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    run = ref.model_run(elf, (buf,), 21)
    deep, depth = deepest(run)
    sp = ref.take(run, (1, deep), ())["regs"][2]["value"]
    want = ref.take(run, (1, deep), [capi.snap_range(sp + 2, 30), (guests.HEAP, guests.HEAP + 4)], 4)
    base = [CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)]
    r = subprocess.run(base + ["--snapshot", "1:%d" % deep, "--dump", "0x%x+30" % (sp + 2), "--dump", "0x%x+4" % guests.HEAP, "--frames", "4"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    summary, regs, frames, words = cli_block(r.stdout)
    s = want["summary"]
    assert summary == dict({k: s[k] for k in ("position", "cycles", "shard", "row", "pc", "depth", "unmatched_returns", "no_value", "initial", "untouched")},
                           frames=s["n_frames"], words=s["n_words"])
    assert regs == {capi.REG_NAMES[k]: want["regs"][k]["value"] for k in range(1, 32)}
    assert len(frames) == 4 and [int(f[1], 16) for f in frames] == [f["fn_pc"] for f in want["frames"]]
    assert [int(f[3], 16) for f in frames] == [f["call_pc"] for f in want["frames"]]
    assert words == {c["addr"]: "??" if c["flags"] & capi.DVT_SNAP_NO_VALUE else "%08x" % c["value"] for c in want["words"]}
    assert words[guests.HEAP] == "??" and len(words) == 9 and s["depth"] == depth
    # the exit
    r = subprocess.run(base + ["--snapshot", "exit"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    summary, regs, frames, words = cli_block(r.stdout)
    assert summary["position"] == summary["cycles"] == run.cycles and regs["sp"] == run.reg[2] and words == {}
    assert summary["pc"] == rv32_model.HALT_PC and len(frames) == summary["frames"] == summary["depth"] == 1
    # without the flag every byte is as before
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == f"input len: {len(buf) - 8}\n"
    for bad in (["--snapshot", "nowhere"], ["--snapshot", "1:"], ["--snapshot", "exit", "--dump", "0x400000"], ["--snapshot", "exit", "--dump", "0x400001+0"]):
        assert subprocess.run(base + bad, capture_output=True, text=True).returncode == 1, bad


def test_the_tool_parses_and_prints():
    assert snapshot_guest.parse_at("exit") == capi.SNAP_EXIT and snapshot_guest.parse_at("3:0x10") == (3, 16)
    assert snapshot_guest.parse_dump("0x400002+30") == capi.snap_range(0x400002, 30) == (0x400000, 0x400020)
    for bad in ("3", ":4", "3:", "nowhere"):
        with pytest.raises(ValueError):
            snapshot_guest.parse_at(bad)
    for bad in ("0x400000", "0x400000+0"):
        with pytest.raises(ValueError):
            snapshot_guest.parse_dump(bad)
    # the lines of sha256_straddling at the exit: ?? for exactly the NO_VALUE cells, * for the INITIAL ones, four words a line
    run = run_of("sha256_straddling")
    ranges = tight_ranges(run)
    snap = host_snapshot("sha256_straddling", ref.EXIT, ranges)
    lines = snapshot_guest.format_snapshot(snap, ranges)
    words = [w for l in lines if l.startswith("  0x") for w in l.split(": ", 1)[1].replace("*", "").split()]
    assert words == ["??" if c["flags"] & capi.DVT_SNAP_NO_VALUE else "%08x" % c["value"] for c in snap["words"]]
    assert lines[0].startswith("after the last instruction") and sum(l.count("*") for l in lines if l.startswith("  0x")) == snap["summary"]["initial"]
    assert lines[-1].strip().startswith("?? : %d words" % snap["summary"]["no_value"])
