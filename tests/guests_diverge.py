"""Guests of the divergence tests (tools/rvasm.py): small programs that read the words of ONE stdin buffer through HINT_LEN /
HINT_READ into the heap and let them decide what runs.  Each shape exists because the stop or the rejoin of csrc/diverge.h can
get it wrong: arms of different lengths, a call on one side only, frames of different depths, one run that ends early, one that
traps.  words(*w) packs an input."""
import struct

from tests.guests import HEAP, _write_pv
from tools.rvasm import Asm, SYS_HINT_LEN, SYS_HINT_READ

STACK_WORDS = 256
MAGIC = 0x600DF00D


def words(*w):
    return struct.pack("<%dI" % len(w), *w)


def _begin():
    """(asm, address of a committed word, top of the stack); the input is read to HEAP, s2 = HEAP, s3 = its end"""
    a = Asm()
    word = a.dword("word", [0])
    stack = a.dword("stack", [0] * STACK_WORDS)
    a.j("main")
    return a, word, stack + 4 * STACK_WORDS


def _read_input(a, sp):
    a.li("sp", sp)
    a.li("t0", SYS_HINT_LEN)
    a.ecall()                      # t0 <- length
    a.mv("s1", "t0")
    a.li("a0", HEAP)
    a.mv("a1", "s1")
    a.li("t0", SYS_HINT_READ)
    a.ecall()
    a.li("s2", HEAP)
    a.add("s3", "s2", "s1")


def _end(a, word, code=0):
    a.li("s5", word)
    a.sw("a0", "s5", 0)
    _write_pv(a, "s5", 4)
    a.halt(code)
    return a.elf()


def branchy():
    """Per input word an if / else on its parity: the odd arm is three instructions, the even arm seven and calls `mix`.  Two
    inputs that differ in the parity of a word split at that word's beq, and rejoin at `next` after arms of different lengths,
    one of them through a call."""
    a, word, sp = _begin()
    a.label("mix")                 # a0 = a0 * 5 + a4
    a.slli("t1", "a0", 2)
    a.add("a0", "a0", "t1")
    a.add("a0", "a0", "a4")
    a.ret()
    a.label("main")
    _read_input(a, sp)
    a.li("a0", 1)
    a.beq("s2", "s3", "done")
    a.label("loop")
    a.lw("a4", "s2", 0)
    a.andi("t2", "a4", 1)
    a.beq("t2", "zero", "even")
    a.xor("a0", "a0", "a4")        # odd
    a.addi("a0", "a0", 3)
    a.j("next")
    a.label("even")
    a.srli("a4", "a4", 1)
    a.call("mix")
    a.addi("a0", "a0", 1)
    a.call("mix")
    a.xori("a0", "a0", 0x55)
    a.label("next")
    a.addi("s2", "s2", 4)
    a.bltu("s2", "s3", "loop")
    a.label("done")
    return _end(a, word)


def depths():
    """Per input word a linear recursion (word & 7) deep: two inputs that differ there split inside `rec`, at frames of different
    depths, and rejoin only below the frame the split happened in or at its base case."""
    a, word, sp = _begin()
    a.label("rec")                 # a1 = levels below this one
    a.addi("sp", "sp", -8)
    a.sw("ra", "sp", 4)
    a.sw("a1", "sp", 0)
    a.addi("a0", "a0", 7)
    a.beq("a1", "zero", "rec_base")
    a.addi("a1", "a1", -1)
    a.call("rec")
    a.xori("a0", "a0", 9)
    a.label("rec_base")
    a.lw("ra", "sp", 4)
    a.addi("sp", "sp", 8)
    a.ret()
    a.label("main")
    _read_input(a, sp)
    a.li("a0", 0)
    a.beq("s2", "s3", "done")
    a.label("loop")
    a.lw("a4", "s2", 0)
    a.andi("a1", "a4", 7)
    a.call("rec")
    a.add("a0", "a0", "a4")
    a.addi("s2", "s2", 4)
    a.bltu("s2", "s3", "loop")
    a.label("done")
    return _end(a, word)


def gate(code=3, tail=40):
    """Halts early with exit code `code` when word 0 is MAGIC, else sums the words `tail` times over and exits 0."""
    a, word, sp = _begin()
    a.label("main")
    _read_input(a, sp)
    a.lw("a4", "s2", 0)
    a.li("t2", MAGIC)
    a.bne("a4", "t2", "work")
    a.halt(code)
    a.label("work")
    a.li("a0", 0)
    a.li("s4", tail)
    a.label("again")
    a.li("s2", HEAP)
    a.label("loop")
    a.lw("a4", "s2", 0)
    a.add("a0", "a0", "a4")
    a.addi("s2", "s2", 4)
    a.bltu("s2", "s3", "loop")
    a.addi("s4", "s4", -1)
    a.bne("s4", "zero", "again")
    return _end(a, word)


def trapper():
    """Sums the words, then loads from HEAP + (word 0 & 3): an input whose word 0 is no multiple of 4 traps there (a misaligned
    lw), after the same instructions as one that does not."""
    a, word, sp = _begin()
    a.label("main")
    _read_input(a, sp)
    a.li("a0", 0)
    a.label("loop")
    a.lw("a4", "s2", 0)
    a.add("a0", "a0", "a4")
    a.addi("s2", "s2", 4)
    a.bltu("s2", "s3", "loop")
    a.li("s2", HEAP)
    a.lw("a4", "s2", 0)
    a.andi("a4", "a4", 3)
    a.add("s2", "s2", "a4")
    a.lw("a5", "s2", 0)            # traps when word 0 & 3
    a.add("a0", "a0", "a5")
    for k in range(20):
        a.addi("a0", "a0", k)
    return _end(a, word)
