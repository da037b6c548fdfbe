"""Guests of the call-tree tests (tools/rvasm.py).  Each shape exists because a span of 4096 records or a shard boundary can
break it; every guest ends with the commit_only ending (tests/guests._write_pv) and HALT(0)."""
from tests.guests import _write_pv
from tools.rvasm import Asm

STACK_WORDS = 1024
FANOUT_STUBS = 129


def _begin():
    """(asm, address of a committed word); sp at the top of a stack in the data segment"""
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    stack = a.dword("stack", [0] * STACK_WORDS)
    a.j("main")
    return a, word, stack + 4 * STACK_WORDS


def _end(a, word):
    a.li("s5", word)
    _write_pv(a, "s5", 4)
    a.halt(0)
    return a.elf()


def _push_ra(a):
    a.addi("sp", "sp", -4)
    a.sw("ra", "sp", 0)


def _pop_ra_ret(a):
    a.lw("ra", "sp", 0)
    a.addi("sp", "sp", 4)
    a.ret()


def nest(rounds=2, leaf_iters=3000):
    """main -> top -> mid -> leaf.  The long leaf loop (3 leaf_iters cycles without an event) makes one frame cover whole spans,
    and at 2^10 cycles per shard its frame opens in shard k and closes after shard k + 2; mid calls leaf a second time, short."""
    a, word, sp = _begin()
    a.label("leaf")                      # a1 = iterations
    a.label("leaf_loop")
    a.addi("a1", "a1", -1)
    a.add("a0", "a0", "a1")
    a.bne("a1", "zero", "leaf_loop")
    a.ret()
    a.label("mid")
    _push_ra(a)
    a.li("a1", leaf_iters)
    a.call("leaf")
    a.addi("a0", "a0", 3)
    a.li("a1", 5)
    a.call("leaf")
    _pop_ra_ret(a)
    a.label("top")
    _push_ra(a)
    a.li("s0", rounds)
    a.label("top_loop")
    a.call("mid")
    a.addi("s0", "s0", -1)
    a.bne("s0", "zero", "top_loop")
    _pop_ra_ret(a)
    a.label("main")
    a.li("sp", sp)
    a.li("a0", 0)
    a.call("top")
    return _end(a, word)


def recurse(depth=320, body=30):
    """Linear recursion `depth` deep with `body` instructions before and after the call: the descent fills several spans with
    unmatched calls only, the ascent with unmatched returns only."""
    assert 2 * (depth + 2) <= STACK_WORDS
    a, word, sp = _begin()
    a.label("rec")                       # a1 = levels below this one
    a.addi("sp", "sp", -8)
    a.sw("ra", "sp", 4)
    a.sw("a1", "sp", 0)
    for k in range(body):
        a.addi("a0", "a0", k & 7)
    a.beq("a1", "zero", "rec_base")
    a.addi("a1", "a1", -1)
    a.call("rec")
    for k in range(body):
        a.xori("a0", "a0", k & 15)
    a.label("rec_base")
    a.lw("ra", "sp", 4)
    a.addi("sp", "sp", 8)
    a.ret()
    a.label("main")
    a.li("sp", sp)
    a.li("a0", 0)
    a.li("a1", depth)
    a.call("rec")
    return _end(a, word)


def dense(n=80, unroll=64):
    """`call f` / `f: ret` back to back, `unroll` of them per loop iteration: almost every record is an event."""
    a, word, sp = _begin()
    a.label("f")
    a.ret()
    a.label("main")
    a.li("s0", n)
    a.label("loop")
    for _ in range(unroll):
        a.call("f")
    a.addi("s0", "s0", -1)
    a.bne("s0", "zero", "loop")
    return _end(a, word)


def tail():
    """f tail-jumps (jal x0) to g and g returns: the frame is f's and g is no function.  h is called through `jalr ra, t0`."""
    a, word, sp = _begin()
    a.label("g")
    a.addi("a0", "a0", 5)
    a.ret()
    a.label("f")
    a.addi("a0", "a0", 1)
    a.j("g")
    a.label("h")
    a.addi("a0", "a0", 2)
    a.ret()
    a.label("main")
    a.li("a0", 0)
    a.call("f")
    a.li("t0", a.labels["h"])
    a.jalr("ra", "t0", 0)
    a.call("f")
    return _end(a, word)


def stray():
    """The entry loads ra by hand and executes `ret` with only the root on the stack (one unmatched return), then halts from
    three calls deep (four frames open at the exit, the root included)."""
    a, word, sp = _begin()
    a.label("after")
    a.call("fa")
    a.label("main")
    a.li("ra", a.labels["after"])
    a.ret()
    a.label("fa")
    a.addi("a0", "a0", 1)
    a.call("fb")
    a.label("fb")
    a.addi("a0", "a0", 2)
    a.call("fc")
    a.label("fc")
    return _end(a, word)


def fanout(rounds=2):
    """129 distinct callees through a table of two-instruction stubs, as guests_profile.jump_table calls its 64."""
    a, word, sp = _begin()
    a.label("stubs")
    for i in range(FANOUT_STUBS):
        a.addi("a0", "a0", i & 15)
        a.ret()
    a.label("main")
    a.li("s2", a.labels["stubs"])
    a.li("s1", FANOUT_STUBS)
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
    return _end(a, word)


def boundary(period=1024):
    """Straight-line padding so that the `call f` is record period - 1 and f's `ret` record 2 period - 1: at 2^10 cycles per
    shard the last record of shard 0 is a CALL and the last record of shard 1 a RET."""
    a = Asm()
    word = a.dword("word", [0x0badc0de])
    for k in range(period - 1):
        a.addi("a0", "a0", k & 3)
    a.call("f")
    a.li("s5", word)
    _write_pv(a, "s5", 4)
    a.halt(0)
    a.label("f")
    for k in range(period - 1):
        a.addi("a1", "a1", k & 3)
    a.ret()
    return a.elf()


GUESTS = {"nest": nest, "recurse": recurse, "dense": dense, "tail": tail, "stray": stray, "fanout": fanout, "boundary": boundary}
