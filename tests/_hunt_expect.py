"""What the forgery hunt (dvt_stage_hunt_cells / dvt_stage_hunt_pairs) must answer, from the CPU oracle alone (test
infrastructure).  A forgery is a list of changes (col, row, delta) of the main trace; it is CAUGHT when

  (a) a unit of the chip is violated on a touched row where it is active (tests/_check_expect.violated_units over the
      touched rows {row - 1, row} mod n of the changed cells), or
  (b) the touched rows' signed multiset of (bus, values) over their interactions with non-zero multiplicity differs from the
      honest table's (the RowEval interpreter of tests/test_soundness_pairs.py over the AIR description).

The honest rows' multisets are computed once per table and row and shared by every forgery that touches the row."""
import collections
import functools

import numpy as np

from tests import _check_expect as ex
from tests.test_soundness_pairs import RowEval

P = 2013265921
DELTAS6 = [1, P - 1, 256, P - 256, 2, 0x78]   # those of the CPU hunter (tests/test_soundness_pairs.py)


@functools.lru_cache(maxsize=None)
def row_eval(machine, cid):
    return RowEval(ex.chip(machine, cid)["desc"])


def _multiset(counters):
    tot = collections.Counter()
    for c in counters:
        tot.update(c)
    return {k: v for k, v in tot.items() if v}


class Table:
    """one honest chip table: canonical column-major main [main_w][n] and prep [prep_w][n], and its public values"""

    def __init__(self, machine, cid, main, prep, pubs):
        self.machine, self.cid = machine, cid
        self.main = np.ascontiguousarray(main, np.uint32).copy()
        n = self.main.shape[1]
        self.prep = np.ascontiguousarray(prep, np.uint32) if prep is not None and prep.shape[0] else np.zeros((0, n), np.uint32)
        self.pubs = [int(x) for x in pubs]
        self.n, self.main_w = n, self.main.shape[0]
        self.info = ex.chip(machine, cid)
        self.ev = row_eval(machine, cid) if self.info["ni"] else None
        self._honest = {}

    def touched(self, changes):
        return sorted({(r + d) % self.n for _, r, _ in changes for d in (-1, 0)})

    def _honest_row(self, r):
        if r not in self._honest:
            self._honest[r] = self.ev.tuples(self.main, self.prep, self.pubs, r)
        return self._honest[r]

    def caught(self, changes):
        """is the table with these changes rejected?  (the cells of `changes` are different cells)"""
        assert len({(c, r % self.n) for c, r, _ in changes}) == len(changes)
        rows = self.touched(changes)
        old = [int(self.main[c, r % self.n]) for c, r, _ in changes]
        try:
            for (c, r, d), v in zip(changes, old):
                self.main[c, r % self.n] = (v + int(d)) % P
            if ex.violated_units(self.machine, self.cid, self.main, self.prep, self.pubs, rows=rows):
                return True
            if self.ev is None:
                return False
            forged = _multiset(self.ev.tuples(self.main, self.prep, self.pubs, r) for r in rows)
        finally:
            for (c, r, _), v in zip(changes, old):
                self.main[c, r % self.n] = v
        return forged != _multiset(self._honest_row(r) for r in rows)

    def free_map(self, deltas, rows, cols=None):
        """[n_deltas][n_cols][len(rows)] of 0 / 1: the single change escapes"""
        cols = range(self.main_w) if cols is None else cols
        return np.array([[[0 if self.caught([(c, r, d)]) else 1 for r in rows] for c in cols] for d in deltas], np.uint8)

    def pairs(self, deltas, row, cols=None, adjacent=False, free=None):
        """The hunt of the pairs with base row `row`: (reported, n_tried).  reported: sorted list of
        (row, c0, c1, d0, d1, alone), alone bit i = change i is caught on its own.  Pairs of two free cells are not
        evaluated; a pair is reported when it escapes."""
        cols = sorted(set(range(self.main_w) if cols is None else cols))
        r1 = (row + 1) % self.n if adjacent else row
        f0 = {(c, d): not self.caught([(c, row, d)]) for c in cols for d in deltas}
        f1 = f0 if r1 == row else {(c, d): not self.caught([(c, r1, d)]) for c in cols for d in deltas}
        reported, tried = [], 0
        for i, c0 in enumerate(cols):
            for c1 in (cols if adjacent else cols[i + 1:]):
                if (c0, row) == (c1, r1):
                    continue
                for d0 in deltas:
                    for d1 in deltas:
                        if f0[(c0, d0)] and f1[(c1, d1)]:
                            continue
                        tried += 1
                        if not self.caught([(c0, row, d0), (c1, r1, d1)]):
                            reported.append((row, c0, c1, d0, d1, (0 if f0[(c0, d0)] else 1) | (0 if f1[(c1, d1)] else 2)))
        return sorted(reported), tried


def caught(machine, cid, main, prep, pubs, changes):
    """one forgery of one table (for many forgeries of a table keep a Table)"""
    return Table(machine, cid, main, prep, pubs).caught(changes)


def n_tried_from_map(fmap0, fmap1, n_cols, adjacent, same_cell=False):
    """pairs the free x free rule leaves, from the single-cell maps [n_deltas][n_cols] of the two rows (0 / 1 = free)"""
    tried = 0
    for c0 in range(n_cols):
        for c1 in (range(n_cols) if adjacent else range(c0 + 1, n_cols)):
            if same_cell and c0 == c1:
                continue
            nf0, nf1 = int(fmap0[:, c0].sum()), int(fmap1[:, c1].sum())
            tried += fmap0.shape[0] * fmap1.shape[0] - nf0 * nf1
    return tried
