"""Guests of the memory-report tests (tools/rvasm.py): what the stock guests of tests/guests.py do not do to the device pass
of csrc/memreport.hip.  Every guest ends with the commit_only ending (tests/guests._write_pv) and HALT(0)."""
from tests.guests import HEAP, _write_pv
from tools.rvasm import Asm

PAGE = 4096


def _end(a, word):
    a.li("s5", word)
    _write_pv(a, "s5", 4)
    a.halt(0)
    return a.elf()


def many_pages(pages=300):
    """One store to each of `pages` consecutive pages from a loop of four instructions, then one load from each: both loops
    lie inside the first 4096 records, so one workgroup sees more distinct pages than its LDS page cache has slots and the
    conflicts fall through to global atomics."""
    assert 8 * pages + 64 < 4096
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    for op in ("sw", "lw"):
        a.li("s1", HEAP + 8)
        a.li("s2", PAGE)
        a.li("s0", pages)
        a.label("loop_" + op)
        getattr(a, op)("a0", "s1", 0)
        a.add("s1", "s1", "s2")
        a.addi("s0", "s0", -1)
        a.bne("s0", "zero", "loop_" + op)
    return _end(a, word)


def hammer(iters=3000):
    """A tight loop that pushes a frame, stores to and loads from one stack slot and pops the frame: every lane of a wave that
    has an access hits the same word of the same page, and x2 is written twice per round."""
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    stack = a.dword("stack", [0] * 64)
    a.li("sp", stack + 4 * 64)
    a.li("s0", iters)
    a.label("loop")
    a.addi("sp", "sp", -16)
    a.sw("s0", "sp", 4)
    a.lw("a0", "sp", 4)
    a.addi("sp", "sp", 16)
    a.addi("s0", "s0", -1)
    a.bne("s0", "zero", "loop")
    return _end(a, word)


def bit_edges():
    """Byte, halfword and word stores that set all 32 bits of one word of the footprint bitmap (32 consecutive guest words
    from an address that is a multiple of 128), the last bit of the bitmap word before it and the first two of the next."""
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    base = HEAP + 5 * PAGE + 128 * 7
    a.li("s1", base)
    a.li("a0", 0x12345678)
    for k in range(-1, 34):
        getattr(a, ("sw", "sb", "sh")[k % 3])("a0", "s1", 4 * k + (k % 3 == 1) * 3 + (k % 3 == 2) * 2)
    a.lw("a1", "s1", 4 * 31)
    a.lw("a1", "s1", 4 * 32)
    return _end(a, word), base


GUESTS = {"many_pages": many_pages, "hammer": hammer, "bit_edges": lambda: bit_edges()[0]}
