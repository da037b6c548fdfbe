"""What a snapshot must say, twice over from the independent model (oracle/rv32_model.py).

take() is the rule of csrc/snapshot.h written over the rows of the model's shards and the pointers of its precompile events
(tests/_watch_ref._calls, _access): every cell, every frame and the summary, to be compared with same().

state_at() is the independent yardstick: the model run again with max_cycles = g stops with the machine as it is before cycle
g (`reg` and `mem`); agrees() holds a snapshot against it.  Registers must be equal, and every cell that carries a value must
equal the machine's word.  The one exception is the documented one: a word outside the image that nothing accessed before the
position (INITIAL) shows the value the memory argument starts it with, run.first_val, which a hinted word holds in the machine
only from its HINT_READ on."""
import functools

from oracle import rv32_model
from tests import _calltree_ref
from tests._profile_ref import model_run  # noqa: F401  (the tests take the run from here)
from tests._watch_ref import LOAD, STORE, _access, _calls

INITIAL, FROM_BEFORE, FROM_AFTER, F_LOAD, F_STORE, IMAGE, NO_VALUE, UNTOUCHED = 1, 2, 4, 8, 16, 32, 64, 128
EXIT = (0xFFFFFFFF, 0xFFFFFFFF)
SPAN = 4096
CELL_KEYS = ("addr", "value", "flags", "shard", "row", "pc")


@functools.lru_cache(maxsize=None)
def _flat(run):
    """[(shard, row, model row, the words the row's precompile call writes)] in execution order"""
    out = []
    for sh in run.shards:
        calls = _calls(sh)
        for i, r in enumerate(sh["rows"]):
            out.append((sh["index"], i, r, tuple(addr for addr, _, wr in calls.get(i, ()) if wr)))
    return out


def locate(run, g):
    """(shard, row) of global record number g; past the last record: the last shard and its record count"""
    base = 0
    for k, sh in enumerate(run.shards):
        n = len(sh["rows"])
        if g < base + n or k + 1 == len(run.shards):
            return sh["index"], min(g - base, n)
        base += n
    return 1, 0


def global_of(run, at):
    """the number of records before position `at`"""
    return sum(1 for sh in run.shards for i in range(len(sh["rows"])) if (sh["index"], i) < tuple(at))


def _cell(addr, value=0, flags=0, src=None):
    return dict(addr=addr, value=value, flags=flags, shard=src[2] if src else 0, row=src[3] if src else 0, pc=src[4] if src else 0)


def take(run, at, ranges=(), frames=64):
    """dict(summary, regs, words, frames) as capi._snapshot gives it (the summary without ms)"""
    flat, at = _flat(run), tuple(at)
    g = global_of(run, at)
    regs = [_cell(k, flags=INITIAL if k else 0) for k in range(32)]
    for shard, row, r, _ in flat[:g]:
        if r.ins.rd:
            regs[r.ins.rd] = dict(addr=r.ins.rd, value=r.a, flags=FROM_BEFORE, shard=shard, row=row, pc=r.ins.pc)
    watched = set(addr for lo, hi in ranges for addr in range(lo, hi, 4))
    before, after = {}, {}   # word -> (kind, value of that side, shard, row, pc)
    for k, (shard, row, r, written) in enumerate(flat):
        acc = _access(r)
        sides = []
        if acc and acc[1] in watched:
            kind = "store" if acc[0] == STORE else "load"
            sides.append((acc[1], (kind, acc[3] if k < g else acc[2], shard, row, r.ins.pc)))
        for addr in written:
            if addr in watched:
                sides.append((addr, ("pre", 0, shard, row, r.ins.pc)))
        for addr, side in sides:
            if k < g:
                before[addr] = side
            else:
                after.setdefault(addr, side)
    words = []
    for lo, hi in ranges:
        for addr in range(lo, hi, 4):
            B, A = before.get(addr), after.get(addr)
            if B and B[0] in ("store", "load"):
                c = _cell(addr, B[1], FROM_BEFORE | (F_STORE if B[0] == "store" else F_LOAD), B)
            elif A and A[0] in ("store", "load"):
                c = _cell(addr, A[1], FROM_AFTER | (0 if B else INITIAL), A)
            elif not B and addr in run.image_mem:
                c = _cell(addr, run.image_mem[addr], IMAGE | INITIAL)
            else:
                c = _cell(addr, 0, NO_VALUE, B or A)
            if not B and not A:
                c["flags"] |= UNTOUCHED
            words.append(c)
    # the call stack: _calltree_ref.tree()'s walk, stopped before record g
    stack, unmatched = [], 0
    for k, (_, _, r, _) in enumerate(flat[:g]):
        if k == 0:
            stack.append((r.ins.pc, 0))
        ev = _calltree_ref.event_of(r.ins.word)
        if ev == "call" and r.next_pc in run.text:
            stack.append((r.next_pc, k + 1))
        elif ev == "ret":
            if len(stack) > 1:
                stack.pop()
            else:
                unmatched += 1
    out_frames = []
    for fn, opened in reversed(stack[max(0, len(stack) - frames):] if frames else []):
        sh, rw = locate(run, opened)
        call = flat[opened - 1][2] if opened else None
        out_frames.append(dict(fn_pc=fn, call_pc=call.ins.pc if call else 0xFFFFFFFF, open_shard=sh, open_row=rw, ra=call.a if call else 0))
    shard, row = locate(run, g)
    summary = dict(position=g, cycles=len(flat), shard=shard, row=row, pc=flat[g][2].ins.pc if g < len(flat) else run.shards[-1]["next_pc"],
                   depth=len(stack), n_frames=len(out_frames), unmatched_returns=unmatched, n_words=len(words),
                   no_value=sum(1 for c in words if c["flags"] & NO_VALUE), initial=sum(1 for c in words if c["flags"] & INITIAL),
                   untouched=sum(1 for c in words if c["flags"] & UNTOUCHED), shards_total=len(run.shards), text_base=run.text_base,
                   n_instr=run.n_instr, span=SPAN)
    return dict(summary=summary, regs=regs, words=words, frames=out_frames)


@functools.lru_cache(maxsize=None)
def _state(elf, stdin, log_shard, g):
    return rv32_model.Run(elf, list(stdin), log_shard, max_cycles=g)


def state_at(elf, stdin, log_shard, g):
    """the model stopped before cycle g: its `reg` and `mem` are the machine's (the whole run at g = cycles)"""
    return _state(bytes(elf), tuple(bytes(b) for b in stdin), log_shard, g)


def same(got, want, where=""):
    """a snapshot (capi._snapshot's dict) against take()'s: exact integers, cell by cell"""
    gs = {k: v for k, v in got["summary"].items() if k != "ms"}
    assert gs == want["summary"], (where, sorted(set(gs.items()) ^ set(want["summary"].items())))
    for part in ("regs", "words", "frames"):
        assert len(got[part]) == len(want[part]), (where, part, len(got[part]), len(want[part]))
        for k, (a, b) in enumerate(zip(got[part], want[part])):
            assert a == b, (where, part, k, a, b)


def agrees(got, state, run, where=""):
    """a snapshot against the machine of state_at(); run: the whole model run (its image and first_val)"""
    for k in range(32):
        assert got["regs"][k]["value"] == state.reg[k], (where, "x%d" % k, got["regs"][k], state.reg[k])
    n = 0
    for c in got["words"]:
        if c["flags"] & NO_VALUE:
            continue
        n += 1
        if c["value"] == state.mem.get(c["addr"], 0):
            continue
        early = c["flags"] & INITIAL and c["addr"] not in run.image_mem and c["value"] == run.first_val.get(c["addr"])
        assert early, (where, c, state.mem.get(c["addr"], 0))
    return n


def no_value(snap, accessed_only=True):
    """the addresses of the NO_VALUE cells; accessed_only: without the words nothing ever decided (UNTOUCHED), which outside the
    image are NO_VALUE by the rule's last row"""
    return sorted(set(c["addr"] for c in snap["words"] if c["flags"] & NO_VALUE and not (accessed_only and c["flags"] & UNTOUCHED)))
