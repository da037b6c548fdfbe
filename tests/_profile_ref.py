"""What the execution report must say, from the independent model (oracle/rv32_model.py): the rows of the model's shards in
execution order give the four tables.  Mnemonics come from the raw words through the table below (the model folds auipc into
lui and addi into add)."""
import collections
import functools

import numpy as np

from oracle import rv32_model

_BR = {0: "beq", 1: "bne", 4: "blt", 5: "bge", 6: "bltu", 7: "bgeu"}
_LD = {0: "lb", 1: "lh", 2: "lw", 4: "lbu", 5: "lhu"}
_ST = {0: "sb", 1: "sh", 2: "sw"}
_IMM = {0: "addi", 2: "slti", 3: "sltiu", 4: "xori", 6: "ori", 7: "andi"}
_REG = {(0, 0): "add", (0x20, 0): "sub", (0, 1): "sll", (0, 2): "slt", (0, 3): "sltu", (0, 4): "xor", (0, 5): "srl", (0x20, 5): "sra",
        (0, 6): "or", (0, 7): "and", (1, 0): "mul", (1, 1): "mulh", (1, 2): "mulhsu", (1, 3): "mulhu", (1, 4): "div", (1, 5): "divu",
        (1, 6): "rem", (1, 7): "remu"}


def mnemonic(word):
    op, f3, f7 = word & 0x7F, (word >> 12) & 7, word >> 25
    if op in (0x37, 0x17, 0x6F):
        return {0x37: "lui", 0x17: "auipc", 0x6F: "jal"}[op]
    if op == 0x67:
        return "jalr" if f3 == 0 else "unknown"
    if op in (0x63, 0x03, 0x23):
        return {0x63: _BR, 0x03: _LD, 0x23: _ST}[op].get(f3, "unknown")
    if op == 0x13:
        if f3 == 1:
            return "slli" if f7 == 0 else "unknown"
        if f3 == 5:
            return {0: "srli", 0x20: "srai"}.get(f7, "unknown")
        return _IMM[f3]
    if op == 0x33:
        return _REG.get((f7, f3), "unknown")
    if op == 0x0F:
        return "fence"
    return "ecall" if word == 0x73 else "unknown"


def tally(run, positions=None):
    """the report of the model's shards at those positions (None: all): dict(cycles, pc_count (numpy u64 over the text), edges =
    {(from_pc, to_pc): count}, syscalls = {id: count}, opcodes = {name: count}, n_transfers)"""
    shards = run.shards if positions is None else [run.shards[k] for k in positions]
    pc_count = np.zeros(run.n_instr, np.uint64)
    edges, sysc, ops = collections.Counter(), collections.Counter(), collections.Counter()
    for sh in shards:
        for r in sh["rows"]:
            pc_count[(r.ins.pc - run.text_base) // 4] += 1
            ops[mnemonic(r.ins.word)] += 1
            if r.ins.kind == "ecall":
                sysc[r.b] += 1
            # (the last row of a shard carries the shard's next_pc; only HALT's is no instruction of the text)
            if r.next_pc != r.ins.pc + 4 and r.next_pc in run.text:
                edges[(r.ins.pc, r.next_pc)] += 1
    return dict(cycles=int(pc_count.sum()), pc_count=pc_count, edges=dict(edges), syscalls=dict(sysc), opcodes=dict(ops),
                n_transfers=sum(edges.values()))


@functools.lru_cache(maxsize=None)
def _run(elf, stdin, log_shard):
    run = rv32_model.Run(elf, list(stdin), log_shard)
    assert run.halted and not run.error, run.error
    return run


def model_run(elf, stdin=(), log_shard=21):
    return _run(bytes(elf), tuple(bytes(b) for b in stdin), log_shard)


def same_tables(prof, want, where=""):
    """all four tables of a report (capi._profile's dict) against tally()'s"""
    s = prof["summary"]
    assert s["cycles"] == want["cycles"] == int(prof["pc_count"].sum()), (where, s["cycles"], want["cycles"])
    assert np.array_equal(prof["pc_count"], want["pc_count"]), where
    got_edges = {(a, b): c for a, b, c in prof["edges"]}
    assert len(got_edges) == len(prof["edges"]) == s["n_edges"] and prof["edges"] == sorted(prof["edges"]), where
    assert got_edges == want["edges"], (where, sorted(set(got_edges.items()) ^ set(want["edges"].items()))[:8])
    assert prof["syscalls"] == want["syscalls"], (where, prof["syscalls"], want["syscalls"])
    assert prof["opcodes"] == want["opcodes"], (where, prof["opcodes"], want["opcodes"])
    assert s["n_transfers"] == want["n_transfers"] and s["dropped_transfers"] == 0, (where, s)


def flow_law(prof, entry_pc, halt_pc=None):
    """pc_count[i] = [i is the entry] + pc_count[i-1] - (transfers out of i-1) - [i-1 is the HALT instruction] + sum of edges
    into i, from the report's outputs alone.  halt_pc: the instruction that retired last (None: nothing halted)."""
    s, pc = prof["summary"], prof["pc_count"].astype(np.int64)
    tb, n = s["text_base"], s["n_instr"]
    out, into = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    for a, b, c in prof["edges"]:
        out[(a - tb) // 4] += c
        into[(b - tb) // 4] += c
    want = into[:n].copy()
    want[(entry_pc - tb) // 4] += 1
    want[1:] += pc[:-1] - out[:n - 1]
    if halt_pc is not None and (halt_pc - tb) // 4 + 1 < n:
        want[(halt_pc - tb) // 4 + 1] -= 1
    bad = np.nonzero(want != pc)[0]
    assert bad.size == 0, [(hex(tb + 4 * int(i)), int(pc[i]), int(want[i])) for i in bad[:8]]
