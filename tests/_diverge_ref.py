"""What a divergence report must say, from the independent model (oracle/rv32_model.py): the rule of csrc/diverge.h, the rejoin
included, written over the rows of two model runs.  report() gives the dicts capi._diverge gives (the summary without ms,
launched_pairs and batch_pairs), chain() the lock-step segments `--rejoin N` walks, same() compares.

A stream is (rows in execution order, the record counts of its shards).  stream_of(run) takes both from a model run.  The model
keeps no rows of a shard that trapped, so trapped_stream() runs it at one cycle per shard, where every retired row sits in a
finished shard, and cuts the rows into shards of 2^log_shard itself: the words the rule compares (idx, a, b, c, m_prev) do not
depend on the shard size; the timestamps, which do, are not compared."""
import functools

from oracle import rv32_model
from tests import _calltree_ref
from tests._origin_ref import global_of, locate, model_run  # noqa: F401  (the tests take these from here)
from tests._watch_ref import _access

SPAN, MAX_KEEP, MAX_WINDOW, DEFAULT_WINDOW = 4096, 64, 16384, 4096
NONE, NO_REJOIN = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
RD, RS1, RS2, MEM = 1, 2, 4, 8
SPLIT, BAD, END_BOTH, END_A, END_B, LIMIT = 1, 2, 3, 4, 5, 6
ENTRY = (1, 0)


class Stream:
    def __init__(self, rows, sizes, text_base):
        self.rows, self.sizes, self.text_base = rows, sizes, text_base

    def __len__(self):
        return len(self.rows)

    def locate(self, g):
        """snap::locate: (shard, row) of global record g; past the last record: the last shard and its record count"""
        base = 0
        for k, n in enumerate(self.sizes):
            if g < base + n or k + 1 == len(self.sizes):
                return k + 1, min(g - base, n)
            base += n
        return 1, 0

    def global_of(self, at):
        """the number of records before position `at` (positions compare as pairs: one past the end is the end)"""
        return sum(min(n, at[1]) if k + 1 == at[0] else n if k + 1 < at[0] else 0 for k, n in enumerate(self.sizes))


@functools.lru_cache(maxsize=None)
def stream_of(run):
    return Stream([r for sh in run.shards for r in sh["rows"]], [len(sh["rows"]) for sh in run.shards], run.text_base)


def trapped_stream(elf, stdin, log_shard):
    """the stream of a guest that traps (see above)"""
    run = rv32_model.Run(elf, list(stdin), 0)
    assert run.error and not run.halted
    rows = [r for sh in run.shards for r in sh["rows"]]
    assert len(rows) == run.cycles and len(rows) % (1 << log_shard)
    return Stream(rows, [1 << log_shard] * (len(rows) >> log_shard) + [len(rows) % (1 << log_shard)], run.text_base)


def _words(r):
    return r.a, r.b, r.c, (r.m_prev if r.mem is not None else 0)


def _rec(s, g):
    if g >= len(s.rows):
        return None
    r = s.rows[g]
    a, b, c, m = _words(r)
    return dict(pc=r.ins.pc, idx=(r.ins.pc - s.text_base) // 4, a=a, b=b, c=c, m_prev=m)


def _candidates(rows):
    """[(i, pc, level)] of the rejoin walk over `rows`: level 0, or 1 for the one record below"""
    out, d = [], 0
    for i, r in enumerate(rows):
        if d < 0:
            out.append((i, r.ins.pc, 1))
            break
        if d == 0:
            out.append((i, r.ins.pc, 0))
        ev = _calltree_ref.event_of(r.ins.word)
        d += 1 if ev == "call" else -1 if ev == "ret" else 0
    return out


def report(sa, sb, start_a=ENTRY, start_b=ENTRY, max_pairs=0, rejoin=False, window=0, keep=16):
    """dict(summary, regs, first, last) of streams sa, sb"""
    ga, gb = sa.global_of(start_a), sb.global_of(start_b)
    n = min(len(sa) - ga, len(sb) - gb)
    if max_pairs:
        n = min(n, max_pairs)
    regs = [dict(n_diff=0, first_diff=NONE, last_diff=NONE, last_write=NONE, live=0) for _ in range(32)]
    data, stop, mask_or, loads, stores = [], n, 0, 0, 0
    for k in range(n):
        ra, rb = sa.rows[ga + k], sb.rows[gb + k]
        if ra.ins.pc != rb.ins.pc:
            stop = k
            break
        wa, wb = _words(ra), _words(rb)
        mask = sum(bit for bit, x, y in zip((RD, RS1, RS2, MEM), wa, wb) if x != y)
        rd = ra.ins.rd
        if rd:
            regs[rd]["last_write"] = k
            if mask & RD:
                regs[rd]["n_diff"] += 1
                if regs[rd]["first_diff"] == NONE:
                    regs[rd]["first_diff"] = k
                regs[rd]["last_diff"] = k
        if not mask:
            continue
        (sha, rwa), (shb, rwb) = sa.locate(ga + k), sb.locate(gb + k)
        e = dict(k=k, shard_a=sha, row_a=rwa, shard_b=shb, row_b=rwb, idx=(ra.ins.pc - sa.text_base) // 4, pc=ra.ins.pc, mask=mask, dir=0, a_a=wa[0], b_a=wa[1],
                 c_a=wa[2], m_a=wa[3], a_b=wb[0], b_b=wb[1], c_b=wb[2], m_b=wb[3], addr_a=0, before_a=0, after_a=0, addr_b=0, before_b=0, after_b=0)
        aa, ab = _access(ra), _access(rb)
        if aa:
            e.update(dir=aa[0], addr_a=aa[1], before_a=aa[2], after_a=aa[3], addr_b=ab[1], before_b=ab[2], after_b=ab[3])
            loads += aa[0] == 1 and bool(mask & MEM)
            stores += aa[0] == 2 and aa[3] != ab[3]
        data.append(e)
        mask_or |= mask
    for r in regs:
        r["live"] = int(r["last_write"] != NONE and r["last_write"] == r["last_diff"])
    if stop < n:
        reason = SPLIT
    elif ga + n == len(sa) and gb + n == len(sb):
        reason = END_BOTH
    elif ga + n == len(sa):
        reason = END_A
    elif gb + n == len(sb):
        reason = END_B
    else:
        reason = LIMIT
    (ssa, sra), (ssb, srb) = sa.locate(ga + stop), sb.locate(gb + stop)
    win = window or DEFAULT_WINDOW
    s = dict(n_pairs=stop, n_data=len(data), first_data=data[0]["k"] if data else NONE, last_data=data[-1]["k"] if data else NONE, n_load_diffs=loads,
             n_store_diffs=stores, cycles_a=len(sa), cycles_b=len(sb), reason=reason, mask=mask_or, stop_shard_a=ssa, stop_row_a=sra, stop_shard_b=ssb,
             stop_row_b=srb, rejoin_shard_a=NO_REJOIN, rejoin_row_a=NO_REJOIN, rejoin_shard_b=NO_REJOIN, rejoin_row_b=NO_REJOIN, rejoin_skip_a=NO_REJOIN,
             rejoin_skip_b=NO_REJOIN, n_kept=min(keep, len(data)), span=SPAN, window=win, stop_a=_rec(sa, ga + stop), stop_b=_rec(sb, gb + stop),
             prev_a=_rec(sa, ga + stop - 1) if stop else None, prev_b=_rec(sb, gb + stop - 1) if stop else None)
    if rejoin and reason == SPLIT:
        ca, cb = _candidates(sa.rows[ga + stop:ga + stop + win]), _candidates(sb.rows[gb + stop:gb + stop + win])
        matches = [(i + j, i, j) for i, pa, la in ca for j, pb, lb in cb if (pa, la) == (pb, lb)] if len(ca) * len(cb) < 1 << 22 else _matches(ca, cb)
        if matches:
            _, i, j = min(matches)
            (s["rejoin_shard_a"], s["rejoin_row_a"]), (s["rejoin_shard_b"], s["rejoin_row_b"]) = sa.locate(ga + stop + i), sb.locate(gb + stop + j)
            s["rejoin_skip_a"], s["rejoin_skip_b"] = i, j
    kept = min(keep, len(data))
    return dict(summary=s, regs=regs, first=data[:kept], last=data[len(data) - kept:] if kept else [])


def _matches(ca, cb):
    """the same minimum for long candidate lists: only the first j of every (pc, level) can win"""
    first_b = {}
    for j, pb, lb in cb:
        first_b.setdefault((pb, lb), j)
    return [(i + first_b[(pa, la)], i, first_b[(pa, la)]) for i, pa, la in ca if (pa, la) in first_b]


def chain(sa, sb, n, window=0, keep=16, call=None):
    """the lock-step segments of `--rejoin n`: report() from the entry, then from every rejoin, at most n + 1 reports.  call:
    another report function with report()'s keywords (the entry points under test walk the same chain)"""
    call = call or (lambda **kw: report(sa, sb, **kw))
    out, at_a, at_b = [], ENTRY, ENTRY
    for _ in range(n + 1):
        got = call(start_a=at_a, start_b=at_b, rejoin=True, window=window, keep=keep)
        out.append(got)
        s = got["summary"]
        if s["reason"] != SPLIT or s["rejoin_skip_a"] == NO_REJOIN:
            break
        at_a, at_b = (s["rejoin_shard_a"], s["rejoin_row_a"]), (s["rejoin_shard_b"], s["rejoin_row_b"])
    return out


def without(got, *drop):
    return dict(got, summary={k: v for k, v in got["summary"].items() if k not in ("ms", "launched_pairs", "batch_pairs") + drop})


def same(got, want, where=""):
    """a report (capi._diverge's dict) against report()'s: exact integers, dict for dict"""
    gs, ws = without(got)["summary"], want["summary"]
    assert gs == ws, (where, sorted((k, gs.get(k), ws.get(k)) for k in set(gs) | set(ws) if gs.get(k) != ws.get(k)))
    for r, (a, b) in enumerate(zip(got["regs"], want["regs"])):
        assert a == b, (where, "x%d" % r, a, b)
    for part in ("first", "last"):
        assert len(got[part]) == len(want[part]), (where, part, len(got[part]), len(want[part]))
        for k, (a, b) in enumerate(zip(got[part], want[part])):
            assert a == b, (where, part, k, sorted(set(a.items()) ^ set(b.items())))
