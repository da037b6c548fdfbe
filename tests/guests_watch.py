"""Guests of the watchpoint tests (tools/rvasm.py): what the stock guests of tests/guests.py do not do to the rule of
csrc/watch.h.  Every guest ends with the commit_only ending (tests/guests._write_pv) and HALT(0)."""
from tests.guests import HEAP, _write_pv
from tools.rvasm import Asm


def sub_stores():
    """sb at every byte offset and sh at both halfword offsets, each into a word whose other bytes are set and each followed by
    a load of the word: the stock subword guest never stores a byte at offset 2.  The stored register has bits above the byte
    and the half that must not reach memory."""
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    buf = a.dword("buf", [0x11223344, 0x55667788, 0x99aabbcc, 0xddeeff00, 0x10203040, 0x50607080])
    a.li("s1", buf)
    a.li("a0", 0xfedcba98)
    for k in range(4):
        a.sb("a0", "s1", 4 * k + k)
        a.lw("a1", "s1", 4 * k)
    for k in range(2):
        a.sh("a0", "s1", 16 + 4 * k + 2 * k)
        a.lhu("a1", "s1", 16 + 4 * k + 2 * k)
    a.li("s2", HEAP + 64)
    a.sb("a0", "s2", 2)          # into a word nothing touched before
    a.lbu("a2", "s2", 2)
    a.li("s5", word)
    _write_pv(a, "s5", 4)
    a.halt(0)
    return a.elf()
