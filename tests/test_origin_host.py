"""Origin slices on the host (dvt_execute_origin, no GPU) against the rule written over the independent model's rows and
precompile events (tests/_origin_ref.slice_of), dict for dict, and against the two yardsticks that do not depend on the rule:
the producer's record holds the value the consumer's record read (edges_agree), and the root's value is the stopped model's
(root_agrees).  Five guests at 2^10 cycles per shard, the registers a0..a5 and the last accessed words, at the exit and in the
middle, with and without FOLLOW_ADDR; depth prefixes, a guest that traps, the CLI and the tool.  Every comparison is of exact
integers."""
import functools
import os
import subprocess

import pytest

from dvt_circuits_amd import capi
from oracle import rv32_model
from tests import _origin_ref as ref
from tests import guests
from tests._watch_ref import _access, _calls
from tests.test_memory_host import CLI, GOLD
from tests.test_snapshot_host import call_guest, trapping
from tests.test_watch_host import watched
from tools import origin_guest

LOG = 10
NAMES = ("bignum", "u256_ops", "hammer", "sub_stores", "hint_sum")
REGS = [capi.origin_reg(k) for k in range(10, 16)]


@functools.lru_cache(maxsize=None)
def run_of(name, log_shard=LOG):
    elf, stdin = watched(name)
    return ref.model_run(elf, stdin, log_shard)


def last_words(run, g, n=4):
    """the last n distinct words a load, a store or a precompile call accessed before record g, latest first"""
    out = []
    flat = [(r, calls.get(i, ())) for sh in run.shards for calls in [_calls(sh)] for i, r in enumerate(sh["rows"])][:g]
    for r, call in reversed(flat):
        acc = _access(r)
        for addr in ([acc[1]] if acc else []) + [a for a, _, _ in call]:
            if addr not in out:
                out.append(addr)
        if len(out) >= n:
            break
    return out[:n]


def places(run):
    return [ref.EXIT, ref.locate(run, run.cycles // 2)]


def host_slice(name, at, target, log_shard=LOG, **kw):
    elf, stdin = watched(name)
    rc, rep, got, err = capi.execute_origin(elf, list(stdin), at, target, log_shard=log_shard, **kw)
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    return got


@pytest.mark.parametrize("name", NAMES)
def test_host_slices_are_the_models(name):
    run = run_of(name)
    elf, stdin = watched(name)
    assert run.cycles == sum(len(sh["rows"]) for sh in run.shards) and len(run.shards) > 2
    checked = roots = 0
    for at in places(run):
        g = ref.global_of(run, at)
        state = ref.state_at(elf, stdin, LOG, g)
        targets = REGS + [capi.origin_word(a) for a in last_words(run, g)]
        assert 7 <= len(targets) <= 10      # (hammer has touched one word by its middle)
        for target in targets:
            for follow in (False, True):
                where = "%s at %s of %s follow %s" % (name, at, target, follow)
                got = host_slice(name, at, target, follow_addr=follow)
                ref.same(got, ref.slice_of(run, at, target, follow), host=True, where=where)
                n = ref.edges_agree(got, where)
                checked += n
                roots += ref.root_agrees(got, target, state, where)
                s = got["summary"]
                print(where, "nodes", s["n_nodes"], "edges", s["n_edges"], "depth", s["depth"], "cut", s["cut"], "checked", n)
                assert s["position"] == g and s["passes"] == 0
    assert checked > 1000 and roots >= 24, (checked, roots)


def test_calls_leaves_and_sub_word_stores_are_followed():
    """u256_ops from the middle: _CALL nodes with one MEM edge per word they read; sub_stores from a word sb / sh wrote: MEM
    edges out of store nodes to the earlier writers of the word; hint_sum: the hinted words are INITIAL leaves"""
    run = run_of("u256_ops")
    at = ref.locate(run, run.cycles // 2)
    got = host_slice("u256_ops", at, capi.origin_reg("a3"))
    calls = [n for n in got["nodes"] if n["kind"] == ref.CALL]
    assert calls, [n["kind"] for n in got["nodes"]]
    for n in calls:
        ins = got["edges"][n["first_edge"]:n["first_edge"] + n["n_edges"]]
        assert n["n_edges"] >= 16 and all(e["role"] == ref.MEM and e["flags"] & ref.NO_VALUE and e["value"] == 0 for e in ins), n
        assert [e["target"] for e in ins[:8]] == [(n["rs2"] & ~3) + 4 * k for k in range(8)]      # array 0 at a0, first
    leaves = [e for e in got["edges"] if e["flags"] & ref.INITIAL]
    assert leaves and all(e["flags"] & ref.IMAGE and e["to"] == ref.NONE for e in leaves)
    assert any(n["flags"] & ref.UNEXPANDED and n["depth"] == 64 for n in got["nodes"])
    run = run_of("sub_stores")
    subs = [(sh["index"], i, r) for sh in run.shards for i, r in enumerate(sh["rows"]) if r.ins.kind in ("sb", "sh")]
    assert len(subs) == 7      # four sb and two sh into words of the image, one sb into a word nothing touched
    for shard, row, r in subs:
        got = host_slice("sub_stores", (shard, row + 1), capi.origin_word(r.maddr))
        root, first = got["edges"][0], got["nodes"][0]
        assert (first["shard"], first["row"], first["kind"]) == (shard, row, ref.F_STORE) and root["value"] == first["after"] == r.m_val
        mem = [e for e in got["edges"][first["first_edge"]:first["first_edge"] + first["n_edges"]] if e["role"] == ref.MEM]
        word = r.maddr & ~3
        assert len(mem) == 1 and (mem[0]["target"], mem[0]["value"], mem[0]["to"]) == (word, r.m_prev, ref.NONE)      # the bytes it keeps: the word before
        assert mem[0]["flags"] == (ref.INITIAL | ref.IMAGE if word in run.image_mem else ref.INITIAL) and r.m_prev == run.image_mem.get(word, 0)
    run = run_of("hint_sum")
    hinted = sorted(a for a, v in run.first_val.items() if v)
    shard, row, r = next((sh["index"], i, r) for sh in run.shards for i, r in enumerate(sh["rows"]) if r.ins.kind == "lw" and r.maddr in hinted)
    got = host_slice("hint_sum", (shard, row + 1), capi.origin_reg(r.ins.rd))
    load = got["nodes"][0]
    mem = got["edges"][load["first_edge"] + load["n_edges"] - 1]
    assert (load["shard"], load["row"], load["kind"]) == (shard, row, ref.LOAD) and got["edges"][0]["value"] == run.first_val[r.maddr]
    assert (mem["role"], mem["target"], mem["value"], mem["flags"], mem["to"]) == (ref.MEM, r.maddr, run.first_val[r.maddr], ref.INITIAL, ref.NONE)


def test_a_shallower_slice_is_a_prefix():
    """without a cap hit the search is breadth first: the nodes of depth <= a are the same whatever the depth asked for"""
    seen = 0
    for name in ("bignum", "sub_stores"):
        run = run_of(name)
        for at in places(run):
            for target in REGS:
                depths = (0, 1, 3, 6)
                slices = [host_slice(name, at, target, depth=d) for d in depths]
                for d, a, b in zip(depths, slices, slices[1:]):
                    if a["summary"]["cut"] or b["summary"]["cut"]:
                        continue
                    key = lambda n: (n["shard"], n["row"], n["pc"], n["kind"], n["depth"], n["rd_value"])
                    assert [key(n) for n in a["nodes"]] == [key(n) for n in b["nodes"][:len(a["nodes"])]], (name, at, target)
                    assert all(n["depth"] > d for n in b["nodes"][len(a["nodes"]):])
                    assert all(bool(n["flags"] & ref.UNEXPANDED) == (n["depth"] == d) for n in a["nodes"])
                    seen += len(b["nodes"]) > len(a["nodes"])
    assert seen > 10


def test_depth_zero_the_edge_cap_and_an_unwritten_target():
    run = run_of("bignum")
    got = host_slice("bignum", ref.EXIT, capi.origin_reg("a1"), depth=0)
    ref.same(got, ref.slice_of(run, ref.EXIT, capi.origin_reg("a1"), depth=0), host=True)
    assert len(got["nodes"]) == 1 and got["nodes"][0]["flags"] == ref.UNEXPANDED and got["nodes"][0]["n_edges"] == 0 and len(got["edges"]) == 1
    full = ref.slice_of(run, ref.EXIT, capi.origin_reg("a1"))
    wide = next(k for k, q in enumerate(full["level_questions"]) if q >= 8)
    cap = sum(full["level_questions"][:wide]) + full["level_questions"][wide] // 2      # stops in the middle of the first level of eight questions
    got = host_slice("bignum", ref.EXIT, capi.origin_reg("a1"), edges=cap)
    want = ref.slice_of(run, ref.EXIT, capi.origin_reg("a1"), edges=cap)
    ref.same(got, want, host=True)
    ref.edges_agree(got)
    s = got["summary"]
    assert s["n_edges"] <= cap < full["summary"]["n_edges"] and s["unexpanded"] > 0 and s["levels"] == wide + 1
    stopped = [n for n in got["nodes"] if n["flags"] & ref.UNEXPANDED]
    assert len({n["depth"] for n in stopped}) == 2      # the rest of the level that hit the cap, and the level its answers added
    # a register and a word nothing ever wrote
    quiet = next(k for k in range(31, 0, -1) if not any(r.ins.rd == k for sh in run.shards for r in sh["rows"]))
    for target in (capi.origin_reg(quiet), capi.origin_word(guests.HEAP + 0x100000)):
        got = host_slice("bignum", ref.EXIT, target)
        ref.same(got, ref.slice_of(run, ref.EXIT, target), host=True)
        assert got["nodes"] == [] and got["edges"][0]["flags"] & ref.INITIAL and got["edges"][0]["to"] == ref.NONE


def test_a_trapping_guest_is_asked_at_its_trap():
    elf, buf = trapping()
    run = rv32_model.Run(elf)
    assert run.error and not run.halted
    rc, rep, got, err = capi.execute_origin(elf, [], capi.SNAP_EXIT, capi.origin_reg("a0"))
    assert rc == capi.DVT_ERR_GUEST and not rep["halted"] and got["summary"]["position"] == got["summary"]["cycles"] == run.cycles == rep["cycles"]
    root, load = got["edges"][0], got["nodes"][0]
    assert root["value"] == run.reg[10] == 1 and load["kind"] == ref.LOAD and load["addr"] == buf and load["rd_value"] == 1
    mem = got["edges"][load["first_edge"]]
    assert (mem["role"], mem["target"], mem["value"], mem["flags"], mem["to"]) == (ref.MEM, buf, 1, ref.INITIAL | ref.IMAGE, ref.NONE)
    ref.edges_agree(got)
    # the word the guest stored before it trapped: its store, and behind it the load
    rc, rep, got, err = capi.execute_origin(elf, [], capi.SNAP_EXIT, capi.origin_word(guests.HEAP + 4), follow_addr=True)
    assert rc == capi.DVT_ERR_GUEST and got["edges"][0]["value"] == run.mem[guests.HEAP + 4] == 1
    assert [n["kind"] for n in got["nodes"][:1]] == [ref.F_STORE] and ref.LOAD in [n["kind"] for n in got["nodes"]]
    assert ref.edges_agree(got) >= 2


def cli_block(stdout):
    """the --origin block: (dict of the summary line, [node dicts], [edge dicts])"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("origin: "))
    summary = {k: int(v, 0) for k, v in (f.split("=") for f in lines[a].split()[1:])}
    kinds = {"op": 1, "load": 2, "store": 3, "call": 4, "syscall": 5}
    roles = {"root": 0, "addr": 1, "rs1": 2, "rs2": 3, "mem": 4}
    nodes, edges = [], []
    for l in lines[a + 1:]:
        f = l.split()
        kv = dict(x.split("=") for x in f[2:]) if len(f) > 2 else {}
        if f and f[0] == "node":
            shard, row = kv["at"].split(":")
            first, n = kv["edges"].split("+")
            nodes.append(dict(shard=int(shard), row=int(row), pc=int(kv["pc"], 16), kind=kinds[kv["kind"]], depth=int(kv["depth"]), first_edge=int(first),
                              n_edges=int(n), flags=int(kv["flags"], 16), rd_value=int(kv["rd"], 16), rs1=int(kv["rs1"], 16), rs2=int(kv["rs2"], 16),
                              addr=int(kv["addr"], 16), before=int(kv["before"], 16), after=int(kv["after"], 16)))
        elif f and f[0] == "edge":
            shard, row = kv["src"].split(":")
            edges.append({"from": int(kv["from"]) & 0xFFFFFFFF, "to": int(kv["to"]) & 0xFFFFFFFF, "role": roles[kv["role"]], "target": int(kv["target"], 16),
                          "value": int(kv["value"], 16), "flags": int(kv["flags"], 16), "src_shard": int(shard), "src_row": int(row)})
        else:
            break
    return summary, nodes, edges


def cli_agrees(stdout, want, host):
    summary, nodes, edges = cli_block(stdout)
    s = want["summary"]
    assert summary == dict({k: s[k] for k in ("position", "cycles", "shard", "row", "depth", "cut", "unexpanded", "initial", "no_value", "questions", "levels")},
                           nodes=s["n_nodes"], edges=s["n_edges"], passes=0 if host else s["passes"])
    assert nodes == [{k: v for k, v in n.items() if k != "idx"} for n in want["nodes"]]
    assert edges == want["edges"]


def test_cli_execute_origin(tmp_path):
    elf = call_guest("recurse")
    path = tmp_path / "recurse.elf"
    path.write_bytes(elf)
    inp = os.path.join(GOLD, "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    run = ref.model_run(elf, (buf,), 21)
    base = [CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)]
    r = subprocess.run(base + ["--origin", "exit:reg:a0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cli_agrees(r.stdout, ref.slice_of(run, ref.EXIT, capi.origin_reg("a0")), True)
    mid = run.cycles // 2
    word = last_words(run, mid, 1)[0]
    r = subprocess.run(base + ["--origin", "1:%d:word:0x%x" % (mid, word + 1), "--depth", "5", "--nodes", "40", "--follow-addr"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = ref.slice_of(run, (1, mid), capi.origin_word(word), True, 5, 40)
    cli_agrees(r.stdout, want, True)
    assert want["nodes"] and want["summary"]["depth"] <= 5
    # without the flag every byte is as before
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == f"input len: {len(buf) - 8}\n"
    for bad in (["--origin", "exit"], ["--origin", "exit:reg:x0"], ["--origin", "exit:reg:q7"], ["--origin", "1:word:0x10"], ["--origin", "exit:word:"],
                ["--origin", "exit:word:0x38000000"], ["--origin", "exit:reg:a0", "--depth", "65"], ["--origin", "exit:reg:a0", "--nodes", "1025"]):
        assert subprocess.run(base + bad, capture_output=True, text=True).returncode == 1, bad


def test_the_tool_parses_and_prints():
    assert origin_guest.parse_target("a0", None) == capi.origin_reg("a0") == (1, 10) and origin_guest.parse_target("x31", None) == (1, 31)
    assert origin_guest.parse_target(None, "0x400006") == capi.origin_word(0x400006) == (2, 0x400004)
    for bad in (("x0", None), ("zero", None), ("x32", None), ("b1", None), (None, None), ("a0", "0x10")):
        with pytest.raises(ValueError):
            origin_guest.parse_target(*bad)
    for name, target in (("u256_ops", capi.origin_reg("a0")), ("bignum", capi.origin_reg("a1"))):
        run = run_of(name)
        got = host_slice(name, ref.locate(run, run.cycles // 2), target)
        lines = origin_guest.format_origin(got, target[0])
        s = got["summary"]
        assert "%d nodes, %d edges, depth %d" % (s["n_nodes"], s["n_edges"], s["depth"]) in lines[0] and lines[0].startswith("before %d:%d" % (s["shard"], s["row"]))
        assert lines[1].startswith("root a") and len(lines) == 1 + s["n_edges"]      # one line per edge: a node, a reference or a leaf
        tree = lines[1:]
        assert sum(" <- ^ " in l for l in tree) == sum(1 for e in got["edges"] if e["to"] != ref.NONE) - s["n_nodes"]
        assert sum(l.endswith(" <- initial") or l.endswith(" <- image") for l in tree) == s["initial"]
        assert sum(" <- cut -> " in l for l in tree) == s["cut"] and sum(l.endswith(" ...") for l in tree) == s["unexpanded"]
        assert sum(" = ?? <- " in l for l in tree) == s["no_value"]
