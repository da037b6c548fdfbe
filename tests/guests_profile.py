"""Guests of the execution-report tests (tools/rvasm.py): control flow that the other guests do not have."""
from tests.guests import _write_pv
from tools.rvasm import Asm

JUMP_STUBS, JUMP_ROUNDS = 64, 3


def jump_table(rounds=JUMP_ROUNDS):
    """Indirect calls through a table of 64 two-instruction stubs, `rounds` times over: 64 call edges out of one `jalr` and 64
    return edges out of the stubs' (the bounded edge table of the report), then the commit_only ending."""
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    a.j("main")
    a.label("stubs")
    for i in range(JUMP_STUBS):
        a.addi("a0", "a0", i & 15)
        a.ret()
    a.label("main")
    a.li("s2", a.labels["stubs"])
    a.li("s1", JUMP_STUBS)
    a.li("s3", 0)
    a.li("s4", rounds)
    a.li("a0", 0)
    a.label("round")
    a.li("s0", 0)
    a.label("loop")
    a.slli("t0", "s0", 3)
    a.add("t1", "s2", "t0")
    a.jalr("ra", "t1", 0)
    a.addi("s0", "s0", 1)
    a.bne("s0", "s1", "loop")
    a.addi("s3", "s3", 1)
    a.bne("s3", "s4", "round")
    a.li("s5", word)
    _write_pv(a, "s5", 4)
    a.halt(0)
    return a.elf()
