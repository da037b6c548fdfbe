"""The memory report on the host (dvt_execute_memory, no GPU) against the rule written over the independent model's rows and
precompile events (tests/_memory_ref.py): table for table on the stock guests, the guests of tests/guests_memory.py, a guest
that traps, and the CLI's block.  Every comparison is of exact integers."""
import collections
import functools
import os
import subprocess

import pytest

from dvt_circuits_amd import capi
from oracle import rv32_model
from tests import _memory_ref as ref
from tests import guests, guests_memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")
GOLD = os.path.join(ROOT, "tests", "golden")
PAGE = ref.PAGE
HINT = bytes(range(1, 41))


@functools.lru_cache(maxsize=None)
def straddling_sha():
    """sha256_precompiled with the schedule array 128 bytes below a page boundary and the state 16 bytes below a later one:
    both arrays of both precompiles straddle a page, in memory that only the calls access"""
    run = ref.model_run(guests.sha256_precompiled()[0])
    w, st = run.shards[0]["sha_ext"][0]["ptr"], run.shards[0]["sha_cmp"][0]["h_ptr"]
    top = (max(w, st) + 2 * PAGE) & ~(PAGE - 1)
    return guests.sha256_precompiled(w_off=top - 128 - w, h_off=top + 3 * PAGE - 16 - st)[0]


# name -> (elf, stdin buffers)
GUESTS = {
    "arith": lambda: (guests.arith()[0], ()),
    "subword": lambda: (guests.subword()[0], ()),
    "hint_sum": lambda: (guests.hint_sum(), (HINT,)),
    "bignum": lambda: (guests.bignum(40)[0], ()),
    "sha256_straddling": lambda: (straddling_sha(), ()),
    "sha_extend": lambda: (guests.sha_extend()[0], ()),
    "field_ops": lambda: (guests.field_ops()[0], ()),
    "curve_ops": lambda: (guests.curve_ops()[0], ()),
    "u256_ops": lambda: (guests.u256_ops()[0], ()),
    "many_pages": lambda: (guests_memory.many_pages(), ()),
    "hammer": lambda: (guests_memory.hammer(), ()),
    "bit_edges": lambda: (guests_memory.bit_edges()[0], ()),
}


@functools.lru_cache(maxsize=None)
def guest(name):
    return GUESTS[name]()


@functools.lru_cache(maxsize=None)
def want(name):
    """the model's report of the whole execution (the shard size does not enter the rule: one run at the default size)"""
    elf, stdin = guest(name)
    return ref.report(ref.model_run(elf, stdin))


@functools.lru_cache(maxsize=None)
def host(name):
    elf, stdin = guest(name)
    rc, rep, mem, err = capi.execute_memory(elf, list(stdin))
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    return rep, mem


@pytest.mark.parametrize("name", sorted(GUESTS))
def test_host_memory_is_the_models(name):
    elf, stdin = guest(name)
    rep, got = host(name)
    run = ref.model_run(elf, stdin)
    w = want(name)
    print(name, got["summary"], "precompile first touches", w["pre_first"])
    ref.same_report(got, w, name)
    s = got["summary"]
    assert s["cycles"] == rep["cycles"] == run.cycles and s["shards_total"] == 1
    # the five laws of the issue, each from its own source
    assert int(got["first_touch"].sum()) == s["first_touches"]
    assert sum(pg["words"] for pg in got["pages"]) == s["words"]
    prevs = [p for sh in run.shards for ev in sh["sha_ext"] for p in ev["prev"]]
    prevs += [p for sh in run.shards for ev in sh["sha_cmp"] for p in ev["wprev"] + ev["hprev"]]
    prevs += [p for sh in run.shards for ev in sh["big"] for p in ev["aprev"] + ev["bprev"]]
    assert s["words"] - s["first_touches"] == sum(1 for p in prevs if p == (0, 0))
    assert s["mem_init_rows"] == len(run.mem_rows())
    x2 = [r.a for sh in run.shards for r in sh["rows"] if r.ins.rd == 2]
    assert (s["sp_writes"], s["sp_min"], s["sp_max"]) == (len(x2), min(x2, default=0), max(x2, default=0))


def test_what_the_guests_are_there_for():
    """from the model: each shape stresses what its docstring says"""
    # the schedule array and the state of the SHA guest straddle a page, and only the calls access them
    run = ref.model_run(straddling_sha())
    ext, cmp_ = run.shards[0]["sha_ext"][0], run.shards[0]["sha_cmp"][0]
    assert ext["ptr"] // PAGE + 1 == (ext["ptr"] + 252) // PAGE and cmp_["w_ptr"] == ext["ptr"]
    assert cmp_["h_ptr"] // PAGE + 1 == (cmp_["h_ptr"] + 28) // PAGE
    w = want("sha256_straddling")
    assert w["pre_first"] == 64 + 8 and all(p == (0, 0) for p in ext["prev"])
    by_page = {pg["page"]: pg for pg in w["pages"]}
    lo, hi = by_page[ext["ptr"] // PAGE * PAGE], by_page[ext["ptr"] // PAGE * PAGE + PAGE]
    calls = len(run.shards[0]["sha_ext"])
    assert (lo["words"], hi["words"], lo["pre_writes"], hi["pre_writes"]) == (32, 32, 16 * calls, 32 * calls)
    assert (lo["pre_reads"], hi["pre_reads"]) == ((16 + 32) * calls, 32 * calls)
    # many_pages: one span of 4096 records stores to more pages than a workgroup's page cache has slots
    rows = [r for sh in ref.model_run(guests_memory.many_pages()).shards for r in sh["rows"]][:4096]
    assert len(set(r.maddr // PAGE for r in rows if r.ins.kind == "sw")) > capi.MEMORY_LDS_PAGE_SLOTS
    assert len(set(r.maddr // PAGE for r in rows if r.ins.kind == "lw")) > capi.MEMORY_LDS_PAGE_SLOTS
    # hammer: thousands of accesses of one word, and x2 moves between two values
    w = want("hammer")
    rows = [r for sh in ref.model_run(guests_memory.hammer()).shards for r in sh["rows"]]
    hits = collections.Counter((r.maddr & ~3, r.ins.kind) for r in rows if r.ins.kind in ("lw", "sw"))
    (slot, _), n = hits.most_common(1)[0]
    assert n == hits[(slot, "lw")] == hits[(slot, "sw")] == 3000
    assert w["summary"]["sp_writes"] == 6000 + 2 and w["summary"]["sp_max"] == slot - 4 + 16      # (li sp: lui and addi)
    # bit_edges: words -1 .. 33 around a multiple of 128 bytes
    elf, base = guests_memory.bit_edges()
    assert base % 128 == 0
    stored = set(r.maddr & ~3 for sh in ref.model_run(elf).shards for r in sh["rows"] if r.ins.kind in ref.STORES and r.maddr >= base - 4)
    assert stored == set(range(base - 4, base + 4 * 34, 4))
    # hint_sum: every hinted word is first touched by the loop's load
    w = want("hint_sum")
    elf, _ = guest("hint_sum")
    run = ref.model_run(elf, (HINT,))
    loads = [r for sh in run.shards for r in sh["rows"] if r.ins.kind == "lw" and r.maddr >= guests.HEAP]
    assert len(loads) == len(HINT) // 4 and all(r.mem == (0, 0) for r in loads)
    assert int(w["first_touch"][(loads[0].ins.pc - run.text_base) // 4]) == len(HINT) // 4
    # subword: several sub-word accesses share a word
    w = want("subword")
    assert w["summary"]["loads"] + w["summary"]["stores"] > 2 * w["summary"]["words"]


def test_a_trapping_guest_is_filled_up_to_the_trap():
    """the model keeps no rows of the shard that trapped, but its memory state: the footprint is compared with it"""
    a = guests_memory.Asm()
    buf = a.dword("buf", [1, 2, 3, 4])
    a.li("s1", buf)
    a.lw("a0", "s1", 0)
    a.sw("a0", "s1", 8)
    a.li("s2", guests.HEAP)
    a.sw("a0", "s2", 4)
    a.lw("a4", "s1", 1)            # misaligned: traps
    a.halt(0)
    elf = a.elf()
    rc, rep, got, err = capi.execute_memory(elf)
    rc0, rep0, _, err0 = capi.execute(elf)
    assert rc == rc0 == capi.DVT_ERR_GUEST and rep == rep0 and err == err0 and not rep["halted"]
    run = rv32_model.Run(elf)
    assert run.error and not run.halted and run.cycles == rep["cycles"]
    s = got["summary"]
    assert s["cycles"] == rep["cycles"] and (s["loads"], s["stores"], s["first_touches"], s["words"]) == (1, 2, 3, 3)
    assert sorted(run.mem_t) == [buf, buf + 8, guests.HEAP + 4]
    want_pages = sorted(set(addr // PAGE * PAGE for addr in run.mem_t))
    assert [pg["page"] for pg in got["pages"]] == want_pages
    assert [pg["words"] for pg in got["pages"]] == [sum(1 for addr in run.mem_t if addr // PAGE * PAGE == p) for p in want_pages]
    assert s["mem_init_rows"] == len(run.mem_rows()) and s["image_words_accessed"] == 2
    ref.laws(got)
    # the stock traps guest: nothing was accessed before the trap
    rc, rep, got, err = capi.execute_memory(guests.traps())
    assert rc == capi.DVT_ERR_GUEST and got["summary"]["cycles"] == rep["cycles"] and got["pages"] == [] and got["summary"]["words"] == 0
    ref.laws(got)


def test_max_cycles_cuts_the_report():
    elf, _ = guest("hammer")
    rc, rep, got, err = capi.execute_memory(elf, max_cycles=1000)
    assert rc == capi.DVT_ERR_GUEST and rep["cycles"] == got["summary"]["cycles"] == 1000, (rc, rep, err)
    assert 0 < got["summary"]["stores"] < 200 and got["summary"]["sp_writes"] > 300
    ref.laws(got)


def block_of(stdout):
    """the --show-memory block: (dict of the summary line, [(first, last, loads, stores, pre_reads, pre_writes, words)])"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("memory: "))
    summary = {k: int(v, 0) for k, v in (f.split("=") for f in lines[a].split()[1:])}
    ranges = []
    for l in lines[a + 1:]:
        f = l.split()
        if len(f) != 6 or "-" not in f[0]:
            break
        first, last = (int(x, 16) for x in f[0].split("-"))
        ranges.append((first, last) + tuple(int(x) for x in f[1:]))
    return summary, ranges


def ranges_of(pages):
    """runs of consecutive pages merged, as the CLI and tools/profile_guest.py print them"""
    out = []
    for pg in pages:
        row = [pg["page"], pg["page"] + PAGE - 1, pg["loads"], pg["stores"], pg["pre_reads"], pg["pre_writes"], pg["words"]]
        if out and out[-1][1] + 1 == pg["page"]:
            out[-1] = [out[-1][0], row[1]] + [x + y for x, y in zip(out[-1][2:], row[2:])]
        else:
            out.append(row)
    return [tuple(r) for r in out]


SUMMARY_KEYS = ("cycles", "loads", "stores", "pre_reads", "pre_writes", "pre_calls", "words", "first_touches", "image_words",
                "image_words_accessed", "mem_init_rows", "sp_writes", "sp_min", "sp_max")


def test_cli_execute_show_memory(tmp_path):
    path = tmp_path / "hint_sum.elf"
    path.write_bytes(guests.hint_sum())
    inp = os.path.join(GOLD, "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    w = ref.report(ref.model_run(guests.hint_sum(), (buf,)))
    base = [CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)]
    r = subprocess.run(base + ["--show-memory"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    summary, ranges = block_of(r.stdout)
    assert summary == dict({k: w["summary"][k] for k in SUMMARY_KEYS}, pages=w["summary"]["n_pages"])
    assert ranges == ranges_of(w["pages"])
    # runs of consecutive pages are merged: the 300 pages of many_pages are one line
    many = tmp_path / "many_pages.elf"
    many.write_bytes(guests_memory.many_pages())
    r = subprocess.run(base[:-1] + [str(many), "--show-memory"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    pages = want("many_pages")["pages"]
    assert block_of(r.stdout)[1] == ranges_of(pages) and len(ranges_of(pages)) + 299 == len(pages)
    # without the flag every byte is as before, and the other reports come first
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == f"input len: {len(buf) - 8}\n"
    both = subprocess.run(base + ["--show-report", "--show-calls"], capture_output=True, text=True)
    three = subprocess.run(base + ["--show-report", "--show-calls", "--show-memory"], capture_output=True, text=True)
    assert both.returncode == three.returncode == 0 and "memory: " not in both.stdout
    assert three.stdout.startswith(both.stdout) and block_of(three.stdout) == (summary, ranges)
