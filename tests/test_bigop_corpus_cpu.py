"""CPU tests (no GPU) of the extremes corpus of the five big-integer precompile chips (tests/_bigop_corpus.py): the
corpus reaches what it claims to reach — conditions on the INPUTS, checked with plain integers and the Python model
(oracle/rv32_model.py) alone — and on it the product's host rows equal the model's in every cell.  The device's rows are
compared with both in tests/test_gpu_k0_bigop_extremes.py."""
import os
import re
import struct

import numpy as np
import pytest

from dvt_circuits_amd import capi
from oracle import rv32_model
from tests import _bigop_corpus as corpus
from tests import guests
from tests.guests import BLS_P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP256, TOP384 = corpus.TOP256, corpus.TOP384


def test_knuth_d_restatement_divides():
    """the branch-recording restatement against Python's own division, on the digits that make the branches"""
    import random

    rng = random.Random(7)
    pool = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff)
    seen = set()
    for _ in range(3000):
        n, m = 1 + rng.getrandbits(3), 9 + rng.getrandbits(3)
        u = [pool[rng.getrandbits(8) % 5] if rng.getrandbits(2) else rng.getrandbits(32) for _ in range(m)]
        v = [pool[rng.getrandbits(8) % 5] if rng.getrandbits(2) else rng.getrandbits(32) for _ in range(n)]
        if v[-1] == 0:
            continue
        q, r, taken = corpus.knuth_d(u, v)
        ui, vi = (sum(d << (32 * i) for i, d in enumerate(x)) for x in (u, v))
        assert (sum(d << (32 * i) for i, d in enumerate(q)), sum(d << (32 * i) for i, d in enumerate(r))) == divmod(ui, vi)
        seen |= taken
    assert seen == set(corpus.DIV_BRANCHES)


@pytest.mark.parametrize("chip", corpus.CHIPS)
def test_guest_runs_in_model_and_executor(chip):
    """every call of the corpus executes; the results in the guest's output are the plain-integer results of the calls;
    row counts sit just past the 64- and 256-thread workgroups of the device's cells and lookups kernels"""
    cases = corpus.cases(chip)
    lo, hi = (257, 300) if chip == "u256_mul" else (65, 130)
    assert lo <= len(cases) <= hi
    elf, offsets = corpus.guest(chip)
    run = corpus.model_run(chip, 21)
    rc, rep, pv, out, err = capi.execute_io(elf)
    assert rc == 0 and rep["halted"] and not rep["unprovable"] and run.error == "" and run.halted, (err, run.error)
    assert rep["cycles"] == run.cycles and out == run.stdout and pv == run.public_values == guests.checksum(out)
    words = struct.unpack("<%dI" % (len(out) // 4), out)
    name, _, wa, wb = rv32_model.BIG_OPS[cases[0][0]]
    assert name == chip
    for (code, aw, bw), off in zip(cases, offsets):
        _, op, wa, wb = rv32_model.BIG_OPS[code]
        want, _ = rv32_model.big_op(chip, op, list(aw), list(aw) if bw == corpus.ALIAS else list(bw or ()))
        assert list(words[off:off + wa]) == want
    assert len(corpus.model_run(chip, 8).shards) >= 4, "at log_shard_size = 8 the calls must span several shards"
    # the shard of the whole run holds one row per call
    rows = corpus.chip_rows(chip, corpus.model_traces(chip, 21, 0)[0])
    assert rows.shape[1] == len(cases)


def test_u256_corpus_reaches_what_it_claims():
    T = corpus.u256_triples()
    assert len(T) >= 257
    M = lambda m: m or 1 << 256
    assert all(x * y // M(m) < 1 << 264 for x, y, m in T), "every call must be provable"
    nbytes = lambda v: (v.bit_length() + 7) // 8
    for n in range(1, 33):      # every byte length, top byte with and without its high bit
        tops = {(m >> (8 * (n - 1))) >> 7 for _, _, m in T if nbytes(m) == n}
        assert tops == {0, 1}, (n, tops)
    ms = {m for _, _, m in T}
    assert {0, 1, 1 << 255, TOP256} <= ms and any(m and m % 2 == 0 and m & (m - 1) for m in ms), "even moduli, 1, 0, 2^255, 2^256 - 1"
    assert any(m and x * y < m and x * y for x, y, m in T) and any(m and x * y < m and x * y == 0 for x, y, m in T), "quotient 0"
    assert sum(1 for x, y, m in T if m and y == m and x) >= 32, "exact multiples"
    assert all(x * y % m == 0 for x, y, m in T if m and y == m)
    q33 = [x * y // M(m) for x, y, m in T if nbytes(x * y // M(m)) == 33]
    assert len(q33) >= 8 and (1 << 264) - 1 in q33, "quotients of exactly 33 significant bytes, 2^264 - 1 among them"
    assert (TOP256, TOP256, 0) in T and sum(1 for x, y, m in T if x == y == TOP256 and m >= 1 << 248) >= 4
    # the long division of the rows: every branch of Knuth's algorithm D at least once
    seen = {}
    for x, y, m in T:
        for b in corpus.u256_division_branches(x, y, m):
            seen[b] = seen.get(b, 0) + 1
    print("long-division branches over the corpus:", seen)
    assert set(seen) == set(corpus.DIV_BRANCHES), sorted(set(corpus.DIV_BRANCHES) - set(seen))
    # the pinned finds still reach the rare branches, with and without a normalisation shift
    rare = {}
    for x, y, m in corpus.U256_DIVISION_FINDS:
        taken = corpus.u256_division_branches(x, y, m)
        for b in ("correction", "qhat_overflow", "rhat_exit", "add_back"):
            if b in taken:
                rare.setdefault(b, set()).add("shift_zero" in taken)
    assert all(rare.get(b) == {False, True} for b in ("correction", "qhat_overflow", "rhat_exit", "add_back")), rare


def test_field_corpus_reaches_what_it_claims():
    edges = set(corpus.FP_EDGES)
    assert edges == {0, 1, BLS_P - 1, BLS_P, BLS_P + 1, TOP384, (BLS_P + 1) // 2}
    fp, fp2 = corpus.fp_calls(), corpus.fp2_calls()
    assert len(fp) >= 65 and len(fp2) >= 65
    for op in (0, 1, 2):
        pairs = {(x, y) for o, x, y in fp if o == op and y != corpus.ALIAS}
        assert pairs <= {(x, y) for x in edges for y in edges}
        # every edge value on both sides, and every unordered pair of them
        assert all(any((x, y) in pairs or (y, x) in pairs for y in edges) for x in edges)
        assert all((x, y) in pairs or (y, x) in pairs for x in edges for y in edges), op
        assert any(o == op and y == corpus.ALIAS for o, x, y in fp) and any(o == op and y == corpus.ALIAS for o, x, y in fp2)
        quads = [(x[0], x[1], y[0], y[1]) for o, x, y in fp2 if o == op and y != corpus.ALIAS]
        assert len(quads) >= 30 and all(set(q) <= edges | {0} for q in quads)
        for pos in range(4):
            assert {q[pos] for q in quads} >= edges, (op, pos)
    for big in (BLS_P - 1, TOP384):
        for pat in corpus.FP2_SIGN_PATTERNS:
            x0, x1, y0, y1 = (big * b for b in pat)
            assert (2, (x0, x1), (y0, y1)) in fp2
    # both ends of x0 y0 - x1 y1 over 384-bit operands are rows
    vals = [x[0] * y[0] - x[1] * y[1] for o, x, y in fp2 if o == 2 and y != corpus.ALIAS]
    assert max(vals) == TOP384 * TOP384 and min(vals) == -TOP384 * TOP384


@pytest.mark.parametrize("chip", ["bls_g1", "secp_k1"])
def test_curve_corpus_reaches_what_it_claims(chip):
    p = corpus.curve_params(chip)[0]
    assert p % 4 == 3
    adds, doubles = corpus.curve_calls(chip)
    assert len(adds) + len(doubles) >= 65
    for pair in (((p - 1, p - 1), (0, 0)), ((0, 0), (p - 1, p - 1)), ((p - 1, 0), (p - 2, p - 1)), ((0, p - 1), (1, 0))):
        assert pair in adds, pair
    for d in ((p - 1, p - 1), (0, 1), (p - 1, 1), (0, p - 1)):
        assert d in doubles, d
    lams = [corpus.add_slope(a, b, p) for a, b in adds]
    assert {0, 1, p - 1} <= set(lams) and {0, 1, p - 1} <= {corpus.double_slope(d, p) for d in doubles}
    results = [guests.ec_add(a, b, p) for a, b in adds]
    assert any(x3 == 0 and y3 for x3, y3 in results) and any(y3 == 0 and x3 for x3, y3 in results) and (0, 0) in results
    on_curve = lambda pt: (pt[1] ** 2 - pt[0] ** 3 - (4 if chip == "bls_g1" else 7)) % p == 0
    assert sum(1 for a, b in adds if not on_curve(a) and not on_curve(b)) >= 16 and sum(1 for d in doubles if not on_curve(d)) >= 14
    assert any(on_curve(a) and on_curve(b) for a, b in adds) and any(on_curve(d) for d in doubles)
    # coordinates and slopes at 0, 1, p - 1, p - 2 all occur as cells of rows
    coords = {v for a, b in adds for pt in (a, b) for v in pt} | {v for d in doubles for v in d} | {v for r in results for v in r}
    assert {0, 1, p - 1, p - 2} <= coords
    # the rows built to drive the DOUBLE slope identity's carries up: lam and y1 of 0xff bytes under p's top byte
    under = (1 << (8 * ((p.bit_length() + 7) // 8 - 1))) - 1
    assert any(y1 & under == under and corpus.double_slope((x1, y1), p) & under == under for x1, y1 in doubles)


def _design_carry_table():
    """{(chip, identity): (cap, recorded min, recorded max)} from the table in DESIGN.md section 5"""
    out = {}
    for line in open(os.path.join(ROOT, "DESIGN.md")):
        m = re.match(r"^\s*\| `(\w+)` \| `(\w+)` \| 2\^(\d+) \| (\d+) \| (\d+) \|", line)
        if m:
            out[(m.group(1), m.group(2))] = (1 << int(m.group(3)), int(m.group(4)), int(m.group(5)))
    return out


def test_carry_cells_of_the_corpus_against_the_recorded_extremes():
    """per identity: the smallest and largest carry cell over the corpus rows (from the model's matrices) against the cell's cap
    and against what DESIGN.md records, so that the corpus cannot quietly get tamer"""
    recorded = _design_carry_table()
    seen = {}
    for chip in corpus.CHIPS:
        _, cdef = corpus.air_chip(chip)
        rows = corpus.chip_rows(chip, corpus.model_traces(chip, 21, 0)[0])
        cells = corpus.carry_cells(chip, rows)
        for rel in cdef.poly_rels:
            cap = 1 << 17 if rel.w_top is not None else 1 << 16
            lo, hi = int(cells[rel.name].min()), int(cells[rel.name].max())
            seen[(chip, rel.name)] = (cap, lo, hi)
            print(f"| `{chip}` | `{rel.name}` | 2^{cap.bit_length() - 1} | {lo} | {hi} |")
            assert 0 <= lo and hi < cap
    assert set(recorded) == set(seen), "DESIGN.md must list every identity of every chip"
    for key, (cap, lo, hi) in seen.items():
        rcap, rlo, rhi = recorded[key]
        assert cap == rcap and hi >= rhi and lo <= rlo, (key, (cap, lo, hi), recorded[key])
    # bls_g1.rel1 is the one identity with a 17th carry bit.  A directed search found no DOUBLE row that sets it:
    # the column is exercised at 0 only, and the corpus keeps the highest carry that search reached
    assert seen[("bls_g1", "rel1")][2] >= 61475
    _, cdef = corpus.air_chip("bls_g1")
    rows = corpus.chip_rows("bls_g1", corpus.model_traces("bls_g1", 21, 0)[0])
    wb = rows[[i for i, n in enumerate(cdef.main_names) if n.startswith("rel1_wb[")]]
    assert wb.shape[0] == 95 and int(wb.max()) == 0


@pytest.mark.parametrize("chip", corpus.CHIPS)
def test_host_rows_equal_the_model_on_the_corpus(chip):
    """capi.rv32_debug_traces against rv32_model.traces: every cell of every chip of the shard (the byte table's
    multiplicities among them) and the public values"""
    elf, _ = corpus.guest(chip)
    host, hpubs, hn = capi.rv32_debug_traces(elf, (), 21, 0)
    model, mpubs = corpus.model_traces(chip, 21, 0)
    assert hn == 1 and (hpubs == mpubs).all()
    assert [c["chip_id"] for c in host] == [c["chip_id"] for c in model]
    assert corpus.air_chip(chip)[0] in [c["chip_id"] for c in host] and corpus.air_chip("byte")[0] in [c["chip_id"] for c in host]
    for h, m in zip(host, model):
        for part in ("main", "prep"):
            assert h[part].shape == m[part].shape, (h["chip_id"], part)
            diff = np.argwhere(h[part] != m[part])
            detail = [(int(c), int(r), int(m[part][c, r]), int(h[part][c, r])) for c, r in diff[:12]]
            assert diff.size == 0, f"chip {h['chip_id']} {part}: {len(diff)} cells differ, first (col,row,model,host): {detail}"
