"""Uses slices on the host (dvt_execute_uses, no GPU) against the rule written over the independent model's rows and precompile
events (tests/_uses_ref.uses_of), dict for dict, and against the three yardsticks that do not depend on the rule: the uses
relation is the inverse of the origin reference's (inverse_of_origin), n_uses is a count over all of the model's rows
(counts_agree), and a consumer's record holds the definition's value (values_agree).  Guests of tests/test_watch_host.watched at
2^10 and 2^14 cycles per shard.  Every property is asserted on the reference's answer inside the test (tests/_uses_ref.shape_of),
so that no case is vacuous; every comparison is of exact integers."""
import functools
import os
import subprocess

import pytest

from dvt_circuits_amd import capi
from tests import _uses_ref as ref
from tests import guests
from tests._watch_ref import _calls
from tests.test_memory_host import CLI, GOLD
from tests.test_snapshot_host import call_guest, trapping
from tests.test_watch_host import hammer_slot, rows_of, watched

S0, A3, SP = (ref.REG, 8), (ref.REG, 13), (ref.REG, 2)


@functools.lru_cache(maxsize=None)
def run_of(name, log_shard=10):
    elf, stdin = watched(name)
    return ref.model_run(elf, stdin, log_shard)


def host_uses(name, at, target, log_shard=10, **kw):
    """the host path's answer, held against the rule and the yardsticks; returns (the rule's answer, its shape)"""
    elf, stdin = watched(name)
    rc, rep, got, err = capi.execute_uses(elf, list(stdin), at, target, log_shard=log_shard, **kw)
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    run = run_of(name, log_shard)
    follow = kw.get("follow_addr", False)
    want = ref.uses_of(run, at, target, follow, kw.get("depth", ref.MAX_DEPTH), kw.get("fan", ref.DEFAULT_FAN), kw.get("nodes", ref.MAX_NODES),
                       kw.get("defs", ref.MAX_DEFS), kw.get("edges", ref.MAX_EDGES))
    ref.check(got, run, want, follow, host=True, where="%s at %s of %s %s" % (name, at, target, kw))
    assert got["summary"]["passes"] == 0
    return want, ref.shape_of(want, run)


@pytest.mark.parametrize("name,log_shard", [("bignum", 10), ("bignum", 14), ("u256_ops", 10), ("hammer", 10), ("sub_stores", 10), ("hint_sum", 10)])
def test_host_slices_are_the_models(name, log_shard):
    run = run_of(name, log_shard)
    assert run.cycles == sum(len(sh["rows"]) for sh in run.shards) and len(run.shards) > 2
    edges = counted = 0
    for at in ((1, 0), ref.locate(run, run.cycles // 3), ref.locate(run, run.cycles // 2), ref.EXIT):
        for target in [(ref.REG, k) for k in (2, 8, 10, 11, 13, 15)]:
            for follow in (False, True):
                want, shape = host_uses(name, at, target, log_shard, follow_addr=follow)
                edges += want["summary"]["n_edges"]
                counted += want["summary"]["uses_total"]
    print(name, log_shard, "edges", edges, "uses", counted)
    assert edges > 100 and counted >= edges


@pytest.mark.parametrize("fan", [1, 8, 16])
def test_fan_keeps_the_first_uses_and_counts_them_all(fan):
    """bignum's loop counter a3: more uses than any fan, from the start of shard 3 and of shard 2"""
    for target, follow in ((A3, False), (A3, True)):
        want, shape = host_uses("bignum", (3, 0), target, 14, fan=fan, follow_addr=follow)
        root = want["defs"][0]
        assert root["n_uses"] > 16 >= fan == root["n_edges"] and root["flags"] & ref.TRUNCATED and "truncated" in shape, root
        wide, _ = host_uses("bignum", (3, 0), target, 14, fan=16, follow_addr=follow)
        first = lambda w, n: [(e["dst_shard"], e["dst_row"], e["role"]) for e in w["edges"][:n]]
        assert first(want, fan) == first(wide, fan) and wide["defs"][0]["n_uses"] == root["n_uses"]      # the same first uses, the same total


def test_dead_live_and_a_next_writer_that_uses_its_target():
    want, shape = host_uses("bignum", (3, 0), (ref.REG, 18), 14)
    assert {"dead", "next_is_use"} <= shape, shape
    dead = [d for d in want["defs"] if not d["n_uses"]]
    assert dead and all(d["n_edges"] == 0 and d["first_edge"] == 0 for d in dead) and want["summary"]["dead"] == len(dead)
    # addi k,k,imm: the next writer of the definition is among its uses
    ended = [d for d in want["defs"] if d["next_shard"] != ref.NONE and any(
        (e["dst_shard"], e["dst_row"]) == (d["next_shard"], d["next_row"]) for e in want["edges"][d["first_edge"]:d["first_edge"] + d["n_edges"]])]
    assert ended and any(want["nodes"][e["to"]]["kind"] == ref.OP for d in ended for e in want["edges"][d["first_edge"]:d["first_edge"] + d["n_edges"]])
    want, shape = host_uses("bignum", (6, 11998), S0, 14, fan=16, follow_addr=True)
    assert {"live_at_exit", "wide_level", "cut"} <= shape, shape
    live = [d for d in want["defs"] if d["flags"] & ref.LIVE_AT_EXIT]
    assert live and all(d["next_shard"] == d["next_row"] == ref.NONE for d in live)


def test_store_load_chains_across_a_shard_edge():
    run = run_of("hammer")
    slot = hammer_slot(run)
    stores = [(s, i, r) for s, i, r in rows_of(run) if r.ins.kind == "sw" and r.maddr & ~3 == slot]
    s, i, r = next(x for x in stores if x[0] == 1 and x[1] > 900)      # late in shard 1
    want, shape = host_uses("hammer", (s, i - 1), (ref.REG, r.ins.rs2))
    kinds = {n["kind"] for n in want["nodes"]}
    assert {ref.OP, ref.F_STORE, ref.LOAD} <= kinds and len({n["shard"] for n in want["nodes"]}) >= 2 and "window_crosses_shard" in shape, (kinds, shape)
    # op -> store -> load: the store's word is read by the load behind it, once, and rewritten by the next store
    store = next(k for k, n in enumerate(want["nodes"]) if n["kind"] == ref.F_STORE)
    word = next(d for d in want["defs"] if d["node"] == store)
    assert (word["what"], word["target"], word["n_uses"], word["value"]) == (ref.WORD, slot, 1, want["nodes"][store]["after"])
    load = want["nodes"][want["edges"][word["first_edge"]]["to"]]
    assert load["kind"] == ref.LOAD and load["before"] == word["value"] and want["edges"][word["first_edge"]]["role"] == ref.MEM
    for follow in (False, True):
        host_uses("hammer", (s, i + 1), (ref.WORD, slot), follow_addr=follow)


def test_store_load_op_store_across_a_shard_edge():
    """bignum's limb loop at 2^10: the word a store writes in shard 3 is loaded in shard 4, the loaded value feeds an op, and the
    op's result is stored again (hammer's loaded value is dead, so that guest has only op -> store -> load)"""
    want, shape = host_uses("bignum", (2, 990), (ref.REG, 6), depth=8)
    chain = ref.store_load_op_store(want)
    assert chain is not None, [n["kind"] for n in want["nodes"]]
    store, load, op, again = (want["nodes"][k] for k in chain)
    assert store["shard"] < load["shard"] == op["shard"] == again["shard"] and "window_crosses_shard" in shape
    assert load["addr"] == store["addr"] and load["before"] == store["after"] and load["rd_value"] in (op["rs1"], op["rs2"]) and again["rs2"] == op["rd_value"]


def test_sub_word_stores_use_and_end_their_word():
    run = run_of("sub_stores")
    subs = [(s, i, r) for s, i, r in rows_of(run) if r.ins.kind in ("sb", "sh")]
    assert len(subs) == 7
    for s, i, r in subs:
        want, shape = host_uses("sub_stores", (1, 0), (ref.WORD, r.maddr & ~3))
        root, first = want["defs"][0], want["nodes"][0]
        assert (root["next_shard"], root["next_row"]) == (s, i) == (first["shard"], first["row"]) and "next_is_use" in shape
        assert first["kind"] == ref.F_STORE and want["edges"][0]["role"] == ref.MEM and root["value"] == r.m_prev == first["before"]
        after = next(d for d in want["defs"] if d["node"] == 0 and d["what"] == ref.WORD)
        assert after["value"] == r.m_val == first["after"]


def test_calls_read_words_and_define_words_without_values():
    run = run_of("u256_ops")
    calls = [(sh["index"], i, c) for sh in run.shards for i, c in sorted(_calls(sh).items())]
    s, i, c = calls[0]
    read = [a for a, rd, wr in c if rd][0]
    want, shape = host_uses("u256_ops", (s, i), (ref.WORD, read))
    call = want["nodes"][0]
    assert call["kind"] == ref.CALL and (call["shard"], call["row"]) == (s, i) and want["edges"][0]["role"] == ref.MEM      # a read word is a MEM use
    assert want["defs"][0]["flags"] & ref.NO_VALUE
    written = [d for d in want["defs"] if d["node"] == 0 and d["what"] == ref.WORD]
    assert [d["target"] for d in written] == [a for a, _, wr in c if wr] and all(d["flags"] & ref.NO_VALUE and d["value"] == 0 for d in written)
    assert "no_value_used" in shape and any(want["nodes"][want["edges"][d["first_edge"]]["to"]]["kind"] == ref.LOAD for d in written if d["n_edges"])


def test_addresses_are_followed_only_when_asked():
    S5 = (ref.REG, 21)      # the pointer bignum's inner loop loads and stores through
    plain, _ = host_uses("bignum", (3, 0), S5, 14, fan=16)
    follow, _ = host_uses("bignum", (3, 0), S5, 14, fan=16, follow_addr=True)
    assert not any(e["role"] == ref.ADDR for e in plain["edges"]) and any(e["role"] == ref.ADDR for e in follow["edges"])
    assert follow["defs"][0]["n_uses"] > plain["defs"][0]["n_uses"]
    mem = [n for n in (follow["nodes"][e["to"]] for e in follow["edges"] if e["role"] == ref.ADDR and e["to"] != ref.NONE)]
    assert mem and all(n["kind"] in (ref.LOAD, ref.F_STORE) for n in mem)


def test_caps_and_depth_zero():
    at = (3, 0)
    full, _ = host_uses("bignum", at, A3, 14)
    want, shape = host_uses("bignum", at, A3, 14, nodes=40)
    cut = [e for e in want["edges"] if e["flags"] & ref.CUT]
    assert cut and all(e["to"] == ref.NONE and e["dst_shard"] >= 3 for e in cut) and want["summary"]["n_nodes"] == 40 < full["summary"]["n_nodes"]
    want, shape = host_uses("bignum", at, A3, 14, defs=30)
    assert want["summary"]["n_defs"] <= 30 < full["summary"]["n_defs"] and want["summary"]["unexpanded"] > 0
    want, shape = host_uses("bignum", at, A3, 14, edges=64)
    assert want["summary"]["n_edges"] <= 64 < full["summary"]["n_edges"] and want["summary"]["unexpanded"] > 0
    stopped = {n["depth"] for n in want["nodes"] if n["flags"] & ref.UNEXPANDED}
    assert len(stopped) == 2      # the rest of the level that hit the cap, and the level its answers added
    want, shape = host_uses("bignum", at, A3, 14, depth=0)
    assert want["summary"]["n_defs"] == 1 and want["nodes"] and all(n["flags"] == ref.UNEXPANDED and n["depth"] == 1 for n in want["nodes"])
    shallow, _ = host_uses("bignum", at, A3, 14, depth=3)
    assert shallow["summary"]["depth"] == 3 and [n["pc"] for n in shallow["nodes"]] == [n["pc"] for n in full["nodes"][:len(shallow["nodes"])]]


def test_the_exit_and_the_first_record_of_a_shard():
    run = run_of("bignum", 14)
    want, shape = host_uses("bignum", ref.EXIT, S0, 14)
    assert want["nodes"] == [] and want["defs"][0]["n_uses"] == 0 and want["defs"][0]["flags"] == ref.LIVE_AT_EXIT | ref.NO_VALUE
    assert want["summary"]["position"] == run.cycles
    first = next((s, i, r) for s, i, r in rows_of(run) if r.ins.kind in ("lw", "lbu", "lhu", "lb", "lh"))
    want, shape = host_uses("bignum", (1, 0), (ref.WORD, first[2].maddr & ~3), 14)      # row 0 of shard 1: the whole execution lies behind
    assert want["summary"]["position"] == 0 and want["nodes"] and (want["nodes"][0]["shard"], want["nodes"][0]["row"]) == first[:2]
    assert want["defs"][0]["value"] == first[2].m_prev
    want, shape = host_uses("bignum", (2, 0), S0, 14, fan=16)
    assert want["summary"]["position"] == len(run.shards[0]["rows"]) and (want["summary"]["shard"], want["summary"]["row"]) == (2, 0) and want["nodes"]


def test_a_trapping_guest_is_followed_to_its_trap():
    elf, buf = trapping()
    row = next(r for r in range(8) if capi.execute_uses(elf, [], (1, r), capi.uses_reg("a0"))[2]["defs"][0]["n_uses"])      # behind lw a0
    rc, rep, got, err = capi.execute_uses(elf, [], (1, row), capi.uses_reg("a0"))
    assert rc == capi.DVT_ERR_GUEST and not rep["halted"] and got["summary"]["cycles"] == rep["cycles"] and got["summary"]["position"] == row
    root = got["defs"][0]
    assert root["n_uses"] == 2 and root["value"] == 1 and root["flags"] == ref.LIVE_AT_EXIT      # both stores read it; nothing wrote a0 again
    assert [(n["kind"], n["rs2"], n["addr"]) for n in got["nodes"]] == [(ref.F_STORE, 1, buf + 8), (ref.F_STORE, 1, guests.HEAP + 4)]
    words = got["defs"][1:]
    assert [(d["what"], d["target"], d["value"], d["n_uses"]) for d in words] == [(ref.WORD, buf + 8, 1, 0), (ref.WORD, guests.HEAP + 4, 1, 0)]
    assert ref.values_agree(got) == 2 and got["summary"]["dead"] == 2 and got["summary"]["live_at_exit"] == 3


def cli_block(stdout):
    """the --uses block: (dict of the summary line, [node dicts], [definition dicts], [edge dicts])"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("uses: "))
    summary = {k: int(v, 0) for k, v in (f.split("=") for f in lines[a].split()[1:])}
    kinds = {"op": 1, "load": 2, "store": 3, "call": 4, "syscall": 5}
    roles = {"addr": 1, "rs1": 2, "rs2": 3, "mem": 4}
    nodes, defs, edges = [], [], []
    pair = lambda t, sep: [int(x) & 0xFFFFFFFF for x in t.split(sep)]
    for l in lines[a + 1:]:
        f = l.split()
        kv = dict(x.split("=") for x in f[2:]) if len(f) > 2 else {}
        if f and f[0] == "node":
            (shard, row), (first, n) = pair(kv["at"], ":"), pair(kv["defs"], "+")
            nodes.append(dict(shard=shard, row=row, pc=int(kv["pc"], 16), kind=kinds[kv["kind"]], depth=int(kv["depth"]), first_def=first, n_defs=n,
                              flags=int(kv["flags"], 16), rd_value=int(kv["rd"], 16), rs1=int(kv["rs1"], 16), rs2=int(kv["rs2"], 16), addr=int(kv["addr"], 16),
                              before=int(kv["before"], 16), after=int(kv["after"], 16)))
        elif f and f[0] == "def":
            (shard, row), (first, n) = pair(kv["next"], ":"), pair(kv["edges"], "+")
            defs.append(dict(n_uses=int(kv["uses"]), node=int(kv["node"]) & 0xFFFFFFFF, what={"reg": 1, "word": 2}[kv["what"]], target=int(kv["target"], 16),
                             value=int(kv["value"], 16), flags=int(kv["flags"], 16), next_shard=shard, next_row=row, first_edge=first, n_edges=n))
        elif f and f[0] == "edge":
            shard, row = pair(kv["dst"], ":")
            edges.append({"def": int(kv["def"]), "to": int(kv["to"]) & 0xFFFFFFFF, "role": roles[kv["role"]], "flags": int(kv["flags"], 16), "dst_shard": shard,
                          "dst_row": row})
        else:
            break
    return summary, nodes, defs, edges


def cli_agrees(stdout, want, host):
    summary, nodes, defs, edges = cli_block(stdout)
    s = want["summary"]
    keys = ("position", "cycles", "shard", "row", "depth", "cut", "unexpanded", "truncated", "live_at_exit", "no_value", "dead", "uses_total", "levels")
    assert summary == dict({k: s[k] for k in keys}, nodes=s["n_nodes"], defs=s["n_defs"], edges=s["n_edges"], passes=0 if host else s["passes"])
    assert nodes == [{k: v for k, v in n.items() if k != "idx"} for n in want["nodes"]]
    assert defs == want["defs"] and edges == want["edges"]


def test_cli_execute_uses(tmp_path):
    elf = call_guest("recurse")
    path = tmp_path / "recurse.elf"
    path.write_bytes(elf)
    inp = os.path.join(GOLD, "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    run = ref.model_run(elf, (buf,), 21)
    base = [CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)]
    mid = run.cycles // 2
    r = subprocess.run(base + ["--uses", "1:%d:reg:sp" % mid, "--follow-addr"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = ref.uses_of(run, (1, mid), SP, True)
    assert {ref.LOAD, ref.OP} <= {n["kind"] for n in want["nodes"]} and any(e["role"] == ref.ADDR for e in want["edges"])
    cli_agrees(r.stdout, want, True)
    load = next(n for n in want["nodes"] if n["kind"] == ref.LOAD)      # the stack word it reads, from the same position on
    r = subprocess.run(base + ["--uses", "1:%d:word:0x%x" % (mid, load["addr"] + 1), "--depth", "5", "--nodes", "40", "--fan", "3"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = ref.uses_of(run, (1, mid), (ref.WORD, load["addr"]), False, 5, 3, 40)
    cli_agrees(r.stdout, want, True)
    assert want["nodes"] and want["nodes"][0]["kind"] == ref.LOAD and want["summary"]["depth"] <= 5
    r = subprocess.run(base + ["--uses", "exit:reg:a0"], capture_output=True, text=True)
    assert r.returncode == 0 and "uses: position=%d " % run.cycles in r.stdout and " nodes=0 defs=1 edges=0 " in r.stdout, r.stderr
    # without the flag every byte is as before
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == f"input len: {len(buf) - 8}\n"
    for bad in (["--uses", "exit"], ["--uses", "exit:reg:x0"], ["--uses", "exit:reg:q7"], ["--uses", "1:word:0x10"], ["--uses", "exit:word:"],
                ["--uses", "exit:word:0x38000000"], ["--uses", "exit:reg:a0", "--depth", "65"], ["--uses", "exit:reg:a0", "--nodes", "1025"],
                ["--uses", "exit:reg:a0", "--fan", "0"], ["--uses", "exit:reg:a0", "--fan", "17"]):
        assert subprocess.run(base + bad, capture_output=True, text=True).returncode == 1, bad


def test_the_tool_prints_the_tree():
    from tools import uses_guest

    for name, at, target, log_shard in (("bignum", (3, 0), A3, 14), ("u256_ops", (1, 24), (ref.WORD, 0x300000), 10)):
        elf, stdin = watched(name)
        got = capi.execute_uses(elf, list(stdin), at, target, log_shard=log_shard, nodes=60)[2]
        lines = uses_guest.format_uses(got)
        s = got["summary"]
        assert "%d nodes, %d definitions, %d edges, depth %d" % (s["n_nodes"], s["n_defs"], s["n_edges"], s["depth"]) in lines[0]
        assert lines[0].startswith("from %d:%d" % (s["shard"], s["row"])) and s["n_nodes"] > 1
        tree = lines[1:]
        assert len(tree) == s["n_defs"] + s["n_edges"]      # one line per definition and one per edge: a node, a reference or a cut
        assert sum(" -> ^ " in l for l in tree) == sum(1 for e in got["edges"] if e["to"] != ref.NONE) - s["n_nodes"]
        assert sum(" -> cut -> " in l for l in tree) == s["cut"] and sum(l.endswith(" ...") for l in tree) == s["unexpanded"]
        assert sum(" = ??, " in l for l in tree) == s["no_value"] and sum(l.endswith(", live") or ", live (+" in l for l in tree) == s["live_at_exit"]
        assert sum(" more)" in l for l in tree) == s["truncated"] and sum(", 0 uses, " in l for l in tree) == s["dead"]
