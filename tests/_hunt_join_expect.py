"""What the join hunt (dvt_stage_hunt_join_*) must answer, from the CPU oracle alone (test infrastructure), on top of
tests/_hunt_expect.Table and the RowEval interpreter.

A candidate is one change (col, row, delta) of a hunted window's table.  Its outcome is

  caught    a unit of the chip is violated on a touched row {row - 1, row} mod n,
  free      the signed multiset of (bus, values) of the touched rows is the honest one,
  absorbed  it differs, but only in tuples that a supply table holds,
  open      it differs in other tuples: D = the exact difference over those, a frozenset of ((bus, values), net mod p).

The supply set is the set of (bus, values) over every interaction of every row of the supply tables, whatever the
multiplicity holds.  A group is a D with the open cells of difference D and those of difference -D; its pairs are the
combinations of one cell of each, except those in the same (tag, chip) at circular row distance <= 1; a group without a pair is
dropped.  Side 0 of a group is the side that holds its lowest cell (tag, chip, row, col, delta); groups are sorted by that
cell, cells inside a side likewise."""
import collections

import numpy as np

from tests import _check_expect as ex
from tests import _hunt_expect as hx

P = hx.P


def all_tuples(table):
    """the set of (bus, values) over every interaction of every row, also where the multiplicity is 0 (all rows at once:
    int64 columns, products of two values below 2^31 fit)"""
    ev, n = table.ev, table.n
    val = {}
    for e in ev.order:
        if e.op == "const":
            v = np.full(n, e.args[0] % P, np.int64)
        elif e.op == "var":
            kind, idx, rot = e.args
            v = np.full(n, int(table.pubs[idx]), np.int64) if kind == "pub" else np.roll((table.main if kind == "main" else table.prep)[idx].astype(np.int64), -rot)
        elif e.op == "neg":
            v = -val[e.args[0].id]
        else:
            x, y = val[e.args[0].id], val[e.args[1].id]
            v = x + y if e.op == "add" else x - y if e.op == "sub" else x * y
        val[e.id] = v % P
    out = set()
    for it in ev.chip.interactions:
        cols = [val[v.id].tolist() for v in it.vals]
        out.update((it.bus, vals) for vals in zip(*cols)) if cols else out.add((it.bus, ()))
    return out


def supply_set(tables):
    out = set()
    for t in tables:
        if t.ev is not None:
            out |= all_tuples(t)
    return out


class Window:
    def __init__(self, tag, table, row_first=0, row_count=None, cols=None):
        self.tag, self.table = tag, table
        self.row_first = row_first
        self.row_count = table.n - row_first if row_count is None else row_count
        self.cols = sorted(set(range(table.main_w) if cols is None else cols))

    def rows(self):
        return range(self.row_first, self.row_first + self.row_count)


def _rows_multiset(t, rows):
    tot = collections.Counter()
    for r in rows:
        tot.update(t.ev.tuples(t.main, t.prep, t.pubs, r))
    return tot


def outcome(t, col, row, delta, supply):
    """("caught" | "free" | "absorbed" | "open", D): D is None unless open"""
    rows = t.touched([(col, row, delta)])
    old = int(t.main[col, row])
    try:
        t.main[col, row] = (old + int(delta)) % P
        if ex.violated_units(t.machine, t.cid, t.main, t.prep, t.pubs, rows=rows):
            return "caught", None
        if t.ev is None:
            return "free", None
        diff = _rows_multiset(t, rows)
    finally:
        t.main[col, row] = old
    for r in rows:
        diff.subtract(t._honest_row(r))
    d_all = {k: v % P for k, v in diff.items() if v % P}
    if not d_all:
        return "free", None
    d = frozenset((k, v) for k, v in d_all.items() if k not in supply)
    return ("open", d) if d else ("absorbed", None)


def negated(d):
    return frozenset((k, P - v) for k, v in d)


def join(windows, deltas, supply_tables=()):
    """dict(candidates, open, absorbed (sorted cells), matched, groups ([side 0, side 1] of sorted cells), pairs); a cell is
    (tag, chip, row, col, delta)"""
    supply = supply_set(supply_tables)
    by, absorbed, n_open, n_cand = collections.defaultdict(list), [], 0, 0
    size = {}
    for w in windows:
        t = w.table
        size[(w.tag, t.cid)] = t.n
        for r in w.rows():
            for c in w.cols:
                for d in deltas:
                    n_cand += 1
                    what, diff = outcome(t, c, r, d, supply)
                    cell = (w.tag, t.cid, r, c, int(d))
                    if what == "absorbed":
                        absorbed.append(cell)
                    elif what == "open":
                        n_open += 1
                        by[diff].append(cell)
    groups, matched, seen = [], 0, set()
    for d, plus in by.items():
        neg = negated(d)
        if d in seen or neg not in by:
            continue
        seen.update((d, neg))
        minus = by[neg]
        matched += len(plus) + len(minus)
        excluded = 0
        for a in plus:
            n = size[a[:2]]
            excluded += sum(1 for b in minus if b[:2] == a[:2] and min((a[2] - b[2]) % n, (b[2] - a[2]) % n) <= 1)
        pairs = len(plus) * len(minus) - excluded
        if not pairs:
            continue
        sides = sorted([sorted(plus), sorted(minus)])
        groups.append((sides, pairs))
    groups.sort(key=lambda g: g[0][0][0])
    return dict(candidates=n_cand, open=n_open, absorbed=sorted(absorbed), matched=matched, groups=[g[0] for g in groups],
                pairs=sum(g[1] for g in groups), distinct=len(by))


def cells_of(side):
    """a side of the product's answer (dicts) as the reference's cells"""
    return [(c["tag"], c["chip"], c["row"], c["col"], c["delta"]) for c in side]


def product_groups(res):
    return [[cells_of(s) for s in g] for g in res["groups"]]
