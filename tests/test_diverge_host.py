"""Divergence reports on the host (dvt_execute_diverge, no GPU) against the rule written over the rows of two runs of the
independent model (tests/_diverge_ref.report), dict for dict: identical inputs, one flipped bit, one word less, guests whose arms
differ in length and depth (the whole chain of segments `--rejoin` walks), a run that exits early, a run that traps, the pair
limit, the keep sizes, the CLI and the tool.  Every comparison is of exact integers, and every property of a shape is asserted
on the reference's answer."""
import functools
import json
import os
import subprocess
import sys

import pytest

from dvt_circuits_amd import capi
from tests import _diverge_ref as ref
from tests import guests, guests_diverge
from tests.test_memory_host import CLI, GOLD, ROOT
from tools import diverge_guest

LOG = 10
INPUT = bytes((37 * k + 11) & 0xFF for k in range(160))      # 40 words
FLIPPED = INPUT[:28] + bytes([INPUT[28] ^ 1]) + INPUT[29:]    # one bit of word 7
SHORTER = INPUT[:-4]
BRANCHY = (guests_diverge.words(1, 2, 3, 4, 5, 6, 7, 8), guests_diverge.words(1, 2, 4, 4, 5, 7, 7, 9))
DEPTHS = (guests_diverge.words(1, 5, 2, 7), guests_diverge.words(1, 3, 2, 0))


@functools.lru_cache(maxsize=None)
def fin_elf():
    return guests.finalization_like(6, INPUT)[0]


@functools.lru_cache(maxsize=None)
def small_elf(name):
    return getattr(guests_diverge, name)()


@functools.lru_cache(maxsize=None)
def stream(elf, stdin, log_shard=LOG):
    return ref.stream_of(ref.model_run(elf, (stdin,), log_shard))


def host(elf, a, b, log_shard=LOG, **kw):
    rc, reps, got, err = capi.execute_diverge(elf, a, b, log_shard=log_shard, **kw)
    assert rc == capi.DVT_OK and got["summary"]["launched_pairs"] == 0, (rc, err)
    return got


def check(elf, a, b, where, log_shard=LOG, **kw):
    """the host path against the rule; returns the rule's answer"""
    want = ref.report(stream(elf, a, log_shard), stream(elf, b, log_shard), **kw)
    ref.same(host(elf, a, b, log_shard, **kw), want, where)
    return want


def test_identical_inputs_and_a_run_against_itself():
    for elf, a in ((fin_elf(), INPUT), (small_elf("branchy"), BRANCHY[0])):
        want = check(elf, a, a, "identical", rejoin=True)
        s = want["summary"]
        assert s["n_data"] == 0 and s["reason"] == ref.END_BOTH and s["n_pairs"] == s["cycles_a"] == s["cycles_b"] and s["mask"] == 0
        assert s["first_data"] == s["last_data"] == ref.NONE and want["first"] == want["last"] == [] and s["stop_a"] is None and s["prev_a"] == s["prev_b"]
        assert all(r["n_diff"] == 0 and not r["live"] and r["first_diff"] == r["last_diff"] == ref.NONE for r in want["regs"])
        assert any(r["last_write"] != ref.NONE for r in want["regs"][1:]) and want["regs"][0]["last_write"] == ref.NONE


def test_one_flipped_bit_is_data_only():
    elf = fin_elf()
    sa = stream(elf, INPUT)
    assert len(sa) == len(stream(elf, FLIPPED)) == 24436 and len(sa.sizes) == 24 and sa.sizes[-1] == 884
    want = check(elf, INPUT, FLIPPED, "one bit of word 7", keep=16)
    s = want["summary"]
    assert s["reason"] == ref.END_BOTH and s["n_pairs"] == 24436 and s["n_data"] > 2 * 64
    first = want["first"][0]
    row = sa.rows[first["k"]]
    assert row.ins.kind == "lw" and first["mask"] == ref.MEM | ref.RD and first["dir"] == 1 and first["addr_a"] == first["addr_b"] == guests.HEAP + 28
    assert first["before_a"] ^ first["before_b"] == 1 and first["k"] == s["first_data"]
    assert s["n_load_diffs"] > 0 and s["n_store_diffs"] > 0 and s["mask"] == 15
    live = [r for r in range(32) if want["regs"][r]["live"]]
    assert live and all(want["regs"][r]["n_diff"] > 0 for r in live)
    print("live", [capi.REG_NAMES[r] for r in live], {k: s[k] for k in ("n_data", "n_load_diffs", "n_store_diffs")})


def test_one_word_less_splits_at_the_loop_and_rejoins():
    elf = fin_elf()
    sa, sb = stream(elf, INPUT), stream(elf, SHORTER)
    assert (len(sa), len(sb)) == (24436, 24423)
    want = check(elf, INPUT, SHORTER, "one word less", rejoin=True)
    s = want["summary"]
    assert s["reason"] == ref.SPLIT and sa.rows[want["first"][0]["k"]].ins.kind == "ecall" and want["first"][0]["k"] == 1      # HINT_LEN's result
    assert want["first"][0]["a_a"] == 160 and want["first"][0]["a_b"] == 156
    prev = sa.rows[s["n_pairs"] - 1]
    assert prev.ins.kind == "bltu" and s["prev_a"]["c"] != s["prev_b"]["c"] and s["prev_a"]["b"] == s["prev_b"]["b"] and prev.ins.rs2 == capi.REG_NAMES.index("s3")
    assert want["regs"][capi.REG_NAMES.index("s3")]["live"] == 1
    assert (s["rejoin_skip_a"], s["rejoin_skip_b"]) == (13, 0)
    again = check(elf, INPUT, SHORTER, "from the rejoin", start_a=(s["rejoin_shard_a"], s["rejoin_row_a"]), start_b=(s["rejoin_shard_b"], s["rejoin_row_b"]),
                  rejoin=True)
    assert again["summary"]["reason"] == ref.END_BOTH and again["summary"]["n_pairs"] == 24436 - s["n_pairs"] - 13
    # the other way round the skips swap
    back = check(elf, SHORTER, INPUT, "B longer", rejoin=True)
    assert (back["summary"]["rejoin_skip_a"], back["summary"]["rejoin_skip_b"]) == (0, 13)
    # without the flag, and with a window that ends before the join, there is none
    assert check(elf, INPUT, SHORTER, "no flag")["summary"]["rejoin_skip_a"] == ref.NO_REJOIN
    assert check(elf, INPUT, SHORTER, "window 13", rejoin=True, window=13)["summary"]["rejoin_skip_a"] == ref.NO_REJOIN
    assert check(elf, INPUT, SHORTER, "window 14", rejoin=True, window=14)["summary"]["rejoin_skip_a"] == 13


@pytest.mark.parametrize("name,inputs", [("branchy", BRANCHY), ("depths", DEPTHS)])
def test_the_chain_of_segments_is_the_models(name, inputs):
    elf = small_elf(name)
    sa, sb = stream(elf, inputs[0]), stream(elf, inputs[1])
    want = ref.chain(sa, sb, 8)
    got = ref.chain(sa, sb, 8, call=lambda **kw: host(elf, inputs[0], inputs[1], **kw))
    assert len(got) == len(want) >= 3
    for k, (g, w) in enumerate(zip(got, want)):
        ref.same(g, w, "%s segment %d" % (name, k))
    shape = [(w["summary"]["rejoin_skip_a"], w["summary"]["rejoin_skip_b"]) for w in want[:-1]]
    print(name, [w["summary"]["n_pairs"] for w in want], shape)
    assert all(w["summary"]["reason"] == ref.SPLIT for w in want[:-1]) and want[-1]["summary"]["reason"] == ref.END_BOTH
    assert all(a != b for a, b in shape)      # arms of different lengths
    # the first split is at the branch on the input word (its parity, its low bits), with the operand differing; the rule takes the
    # smallest i + j, so a later segment may run the two inputs one loop iteration apart: only the chain as a whole is compared
    first = want[0]["summary"]
    assert sa.rows[first["n_pairs"] - 1].ins.kind == "beq" and first["prev_a"]["b"] != first["prev_b"]["b"] and first["prev_a"]["pc"] == first["prev_b"]["pc"]
    assert any(r["live"] for r in want[0]["regs"])


def test_a_run_that_ends_early_and_a_run_that_traps():
    elf = small_elf("gate")
    a, b = guests_diverge.words(guests_diverge.MAGIC, 2, 3), guests_diverge.words(5, 2, 3)
    sa, sb = stream(elf, a), stream(elf, b)
    rc, reps, got, err = capi.execute_diverge(elf, a, b, log_shard=LOG, rejoin=True)
    assert rc == capi.DVT_OK and (reps[0]["exit_code"], reps[1]["exit_code"]) == (3, 0) and reps[0]["halted"], err
    want = ref.report(sa, sb, rejoin=True)
    ref.same(got, want, "gate")
    s = want["summary"]
    assert s["reason"] == ref.SPLIT and s["rejoin_skip_a"] == ref.NO_REJOIN and sa.rows[s["n_pairs"] - 1].ins.kind == "bne"
    assert s["prev_a"]["b"] == guests_diverge.MAGIC and s["prev_b"]["b"] == 5
    # both take the early exit: A (two words) ends first, the third word is never read
    short = guests_diverge.words(guests_diverge.MAGIC, 9)
    assert check(elf, short, a, "gate, both exit")["summary"]["reason"] == ref.END_BOTH
    elf = small_elf("trapper")
    ok, bad = guests_diverge.words(8, 1, 2, 3), guests_diverge.words(9, 1, 2, 3)
    so, st = stream(elf, ok, 4), ref.trapped_stream(elf, (bad,), 4)
    for (x, sx), (y, sy), reason in (((ok, so), (bad, st), ref.END_B), ((bad, st), (ok, so), ref.END_A)):
        rc, reps, got, err = capi.execute_diverge(elf, x, y, log_shard=4, keep=64)
        assert rc == capi.DVT_OK and sorted(r["halted"] for r in reps) == [False, True], err
        want = ref.report(sx, sy, keep=64)
        ref.same(got, want, "trapper")
        s = want["summary"]
        assert s["reason"] == reason and s["n_pairs"] == len(st) < len(so) and s["n_data"] > 0
        assert (s["stop_a"] is None) == (reason == ref.END_A) and (s["stop_b"] is None) == (reason == ref.END_B)
    # the record the other run has at the stop is the load that trapped
    assert so.rows[len(st)].ins.kind == "lw"


@pytest.mark.parametrize("max_pairs", [1, 4096, 4097])
def test_the_pair_limit(max_pairs):
    want = check(fin_elf(), INPUT, FLIPPED, "max_pairs %d" % max_pairs, max_pairs=max_pairs)
    s = want["summary"]
    assert s["reason"] == ref.LIMIT and s["n_pairs"] == max_pairs and (s["stop_a"] is not None) and s["stop_a"]["idx"] == s["stop_b"]["idx"]
    # a limit that is the length of the shorter run is its end
    assert check(fin_elf(), INPUT, SHORTER, "limit at the end", max_pairs=600)["summary"]["reason"] == ref.SPLIT
    assert check(fin_elf(), INPUT, FLIPPED, "limit = length", max_pairs=24436)["summary"]["reason"] == ref.END_BOTH


@pytest.mark.parametrize("keep", [0, 1, 4, 64])
def test_the_keep_sizes(keep):
    many = check(fin_elf(), INPUT, FLIPPED, "keep %d, many" % keep, keep=keep)
    few = check(fin_elf(), INPUT, SHORTER, "keep %d, few" % keep, keep=keep)
    assert many["summary"]["n_data"] > 128 and 4 < few["summary"]["n_data"] == 44 < 64
    assert len(many["first"]) == len(many["last"]) == keep and len(few["first"]) == len(few["last"]) == min(keep, 44)
    if keep == 64:
        assert few["first"] == few["last"] and many["first"][-1]["k"] < many["last"][0]["k"]
    if keep == 4:
        assert few["first"][-1]["k"] < few["last"][0]["k"] and few["last"][-1]["k"] == few["summary"]["last_data"]


def test_later_and_unequal_starts():
    elf = fin_elf()
    sa = stream(elf, INPUT)
    for start in ((2, 0), (3, 17), (24, 883), (24, 884)):
        want = check(elf, INPUT, FLIPPED, "both from %s" % (start,), start_a=start, start_b=start)
        assert want["summary"]["n_pairs"] == len(sa) - sa.global_of(start) and want["summary"]["reason"] == ref.END_BOTH
    # off by one: the runs are out of step at once
    want = check(elf, INPUT, FLIPPED, "out of step", start_a=(1, 5), start_b=(1, 6), rejoin=True)
    assert want["summary"]["reason"] == ref.SPLIT and want["summary"]["n_pairs"] < 8


def cli_blocks(stdout):
    """the blocks of `dvt_prover_host diverge`: [dict(summary fields, live=[names], first=[...], last=[...], recs)]"""
    blocks = []
    for line in stdout.splitlines():
        f = line.split()
        if f[0] == "diverge:":
            kv = dict(x.split("=") for x in f[1:])
            blocks.append(dict(summary=kv, live=None, first=[], last=[], recs={}))
        elif f[0] in ("deciding", "stop"):
            blocks[-1]["recs"][f[0] + " " + f[1].rstrip(":")] = None if f[2] == "none" else {k: int(v, 16) for k, v in (x.split("=") for x in f[2:])}
        elif f[0] == "live:":
            blocks[-1]["live"] = f[1:]
        elif f[0] in ("first", "last"):
            blocks[-1][f[0]].append(line)
    return blocks


def pair_line(part, e):
    line = "%s k=%d at=%d:%d/%d:%d pc=0x%x mask=0x%x a=0x%x/0x%x b=0x%x/0x%x c=0x%x/0x%x m=0x%x/0x%x" % (
        part, e["k"], e["shard_a"], e["row_a"], e["shard_b"], e["row_b"], e["pc"], e["mask"], e["a_a"], e["a_b"], e["b_a"], e["b_b"], e["c_a"], e["c_b"], e["m_a"],
        e["m_b"])
    if e["dir"]:
        line += " %s addr=0x%x/0x%x before=0x%x/0x%x after=0x%x/0x%x" % ("load" if e["dir"] == 1 else "store", e["addr_a"], e["addr_b"], e["before_a"], e["before_b"],
                                                                          e["after_a"], e["after_b"])
    return line


def cli_agrees(stdout, want):
    """the CLI's blocks against a chain of report()s"""
    blocks = cli_blocks(stdout)
    assert len(blocks) == len(want), (len(blocks), len(want))
    num = lambda v: -1 if v in (ref.NONE, ref.NO_REJOIN) else v
    for b, w in zip(blocks, want):
        s = w["summary"]
        assert b["summary"] == dict(
            pairs=str(s["n_pairs"]), reason=capi.DIV_REASONS[s["reason"]], data=str(s["n_data"]), first_data=str(num(s["first_data"])),
            last_data=str(num(s["last_data"])), mask="0x%x" % s["mask"], load_diffs=str(s["n_load_diffs"]), store_diffs=str(s["n_store_diffs"]),
            stop_a="%d:%d" % (s["stop_shard_a"], s["stop_row_a"]), stop_b="%d:%d" % (s["stop_shard_b"], s["stop_row_b"]), cycles_a=str(s["cycles_a"]),
            cycles_b=str(s["cycles_b"]), rejoin_a="%d:%d" % (num(s["rejoin_shard_a"]), num(s["rejoin_row_a"])),
            rejoin_b="%d:%d" % (num(s["rejoin_shard_b"]), num(s["rejoin_row_b"])), skip_a=str(num(s["rejoin_skip_a"])), skip_b=str(num(s["rejoin_skip_b"]))), b["summary"]
        assert b["live"] == [capi.REG_NAMES[r] for r in range(32) if w["regs"][r]["live"]]
        for name, key in (("deciding a", "prev_a"), ("deciding b", "prev_b"), ("stop a", "stop_a"), ("stop b", "stop_b")):
            rec = s[key]
            assert b["recs"][name] == (None if rec is None else dict(pc=rec["pc"], a=rec["a"], b=rec["b"], c=rec["c"], m=rec["m_prev"])), name
        for part in ("first", "last"):
            assert b[part] == [pair_line(part, e) for e in w[part]], part


def test_cli_on_two_share_vectors(tmp_path):
    """`dvt_prover_host diverge --host` on the good 2-to-1 share vector against the one with a bad secret key, through the guest of
    tools/build_guests.py: this input exits 0, that one exits 1"""
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "build_guests.py"), str(tmp_path)], stdout=subprocess.DEVNULL)
    elf = open(os.path.join(str(tmp_path), "bad-share.elf"), "rb").read()
    vec, codes = [], []
    for x in ("", "-bad-secret-key"):      # a vector file holds the scenario, which is the CLI's input, beside its expected exit code
        v = json.load(open(os.path.join(GOLD, "share_vectors", "seeds-commitment-from-2-to-1%s.json" % x)))
        vec.append(str(tmp_path / ("scenario%s.json" % x)))
        codes.append(int(v["params"]["expected_exit_code"]))
        open(vec[-1], "w").write(json.dumps(v["scenario"]))
    assert codes[0] != codes[1]
    bufs = [capi.stdin_from_json("bad-share", open(v, "rb").read()) for v in vec]
    sa, sb = [ref.stream_of(ref.model_run(elf, (b,), 21)) for b in bufs]
    want = ref.chain(sa, sb, 2, keep=4)
    base = [CLI, "diverge", "--type", "bad-share", "-i", vec[0], "--against", vec[1], "--elf", os.path.join(str(tmp_path), "bad-share.elf"), "--host"]
    r = subprocess.run(base + ["--rejoin", "2"], capture_output=True, text=True, timeout=300)
    print(r.stdout[:3000], r.stderr)
    assert r.returncode == 0, r.stderr
    cli_agrees(r.stdout, want)
    assert want[0]["summary"]["n_data"] > 0 and any(w["summary"]["reason"] == ref.SPLIT for w in want)
    one = subprocess.run(base + ["--keep", "2"], capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stderr
    cli_agrees(one.stdout, ref.chain(sa, sb, 0, keep=2))
    for bad in (["--keep", "65"], ["--from", "exit"], ["--from", "9"], ["--against-from", "1"]):
        assert subprocess.run(base + bad, capture_output=True, text=True, timeout=300).returncode == 1, bad
    assert subprocess.run([a for a in base if a not in ("--against", vec[1])], capture_output=True, text=True).returncode == 1


def test_the_tool_prints_and_follows_the_origin(capsys):
    elf = fin_elf()
    got = host(elf, INPUT, SHORTER, rejoin=True)
    lines = diverge_guest.format_report(got)
    s = got["summary"]
    assert lines[0].startswith("%d pairs in step, then split" % s["n_pairs"]) and "%d data pairs" % s["n_data"] in lines[0]
    assert any(l.startswith("deciding A: pc 0x%08x" % s["prev_a"]["pc"]) for l in lines)
    assert any(l.startswith("live:") and " s3" in l for l in lines) and any(l.startswith("rejoin") and "+13" in l for l in lines)
    assert sum(l.startswith("  first") for l in lines) == sum(l.startswith("  last") for l in lines) == s["n_kept"]
    # the differing operand of the deciding branch, followed back: it reaches HINT_LEN's result
    target, slices = diverge_guest.deciding_origins(got, lambda stdin, at, target: capi.execute_origin(elf, [stdin], at, target, log_shard=LOG)[2], INPUT, SHORTER,
                                                     elf)
    assert target == capi.origin_reg("s3")
    for sl, length in zip(slices, (160, 156)):
        assert any(n["kind"] == capi.DVT_ORIGIN_SYSCALL and n["rd_value"] == length for n in sl["nodes"])
