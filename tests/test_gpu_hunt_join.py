"""GPU tests of the join hunt (hunt_join.cuh through Prover.hunt_join / dvt_stage_hunt_join_*) against the CPU reference
(tests/_hunt_join_expect.py: the oracle's constraints on the touched rows and the exact multiset differences): outcome
counts, absorbed cells and groups must be equal, cell by cell.

Shapes: the toy machine at 2^3 fib rows and 2^4 pairs rows with planted rows (an all-zero real row; two distant real rows
whose x differ by one); pairs tables of 2^0, 2^1, 2^2 rows (below four rows every same-table pair is excluded); a window
(3, 11); windows of 65 and 257 rows of a 2^9-row table (the ragged last wave and the ragged last workgroup of the
wave-aggregated record slots); one table under two tags; a hot group of 300 x 300 cells; every capacity one short.  The hot
group's table has 2^10 rows: the 600 real rows it needs do not fit into 2^9."""
import ctypes as C

import numpy as np
import pytest

from tests import _check_expect as ex
from tests import _hunt_expect as hx
from tests import _hunt_join_expect as jx
from tests import toy_traces
from tests.test_gpu_opening_parity import internal

pytestmark = pytest.mark.gpu
P = hx.P
RANGE8, FIB, PAIRS = toy_traces.RANGE8, toy_traces.FIB, toy_traces.PAIRS
X, Y, Z, IS_REAL, MULT = 0, 1, 2, 3, 0
DELTAS4 = [1, P - 1, 3, P - 3]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


# ------------------------------------------------------------------ tables
def pairs_table(log_n, rows):
    """a pairs table of 2^log_n rows: `rows` (x, y, z, is_real) first, padding after"""
    main = np.zeros((4, 1 << log_n), np.uint32)
    for r, row in enumerate(rows):
        main[:, r] = row
    t = hx.Table("toy", PAIRS, main, None, [])
    assert not ex.violated_units("toy", PAIRS, t.main, t.prep, t.pubs), "the planted table is not honest"
    return t


def toy_tables():
    """the three tables of toy_traces.build(log_fib=3, log_pairs=4, real_pairs=11) with three pairs rows planted and the
    multiplicities recomputed: row 1 an all-zero real row, rows 3 and 8 real with y = z = 0 and x = 5 / 6"""
    prep, main, pubs = toy_traces.build(log_fib=3, log_pairs=4, real_pairs=11)
    main, prep = dict(main), dict(prep)
    pairs = main[PAIRS].copy()
    pairs[:, 1], pairs[:, 3], pairs[:, 8] = (0, 0, 0, 1), (5, 0, 0, 1), (6, 0, 0, 1)
    mult = np.zeros(256, np.uint32)
    for v in main[FIB][2]:
        mult[v] += 1
    for r in range(16):
        if pairs[3, r]:
            for v in pairs[:3, r]:
                mult[v] += 1
    tabs = {RANGE8: hx.Table("toy", RANGE8, mult[None, :], prep[RANGE8], []), FIB: hx.Table("toy", FIB, main[FIB], None, pubs),
            PAIRS: hx.Table("toy", PAIRS, pairs, None, [])}
    # honest: no unit violated, and the bus balances
    net = {}
    for t in tabs.values():
        assert not ex.violated_units("toy", t.cid, t.main, t.prep, t.pubs)
        for r in range(t.n):
            for k, v in t.ev.tuples(t.main, t.prep, t.pubs, r).items():
                net[k] = net.get(k, 0) + v
    assert not any(net.values()), "the planted tables do not balance"
    return tabs


@pytest.fixture(scope="module")
def toy():
    return toy_tables()


@pytest.fixture(scope="module")
def toy_all(toy):
    """the reference's answer for all three tables hunted over all rows, no supply table (shared, never changed)"""
    return jx.join([jx.Window(0, toy[c]) for c in (RANGE8, FIB, PAIRS)], DELTAS4)


@pytest.fixture(scope="module")
def toy_supplied(toy):
    """... for fib and pairs hunted with range8 as the supply table"""
    return jx.join([jx.Window(0, toy[c]) for c in (FIB, PAIRS)], [1, P - 1, 256], [toy[RANGE8]])


def dev(gpu, t):
    """a table's device matrices, as Prover.hunt_join takes them"""
    return dict(chip=t.cid, main=internal(gpu, t.main), prep=internal(gpu, t.prep) if t.prep.shape[0] else None, log_n=t.n.bit_length() - 1,
                pubs=t.pubs)


def run(gpu, windows, deltas, supply=(), **kw):
    """Prover.hunt_join over reference windows"""
    ws = [dict(dev(gpu, w.table), tag=w.tag, row_first=w.row_first, row_count=w.row_count, cols=w.cols if len(w.cols) < w.table.main_w else None)
          for w in windows]
    return gpu.hunt_join(windows[0].table.machine, ws, deltas, supply=[dev(gpu, t) for t in supply], **kw)


def check(gpu, windows, deltas, supply=(), want=None, where=""):
    """product against reference: outcome counts, absorbed cells, groups"""
    want = jx.join(windows, deltas, supply) if want is None else want
    got = run(gpu, windows, deltas, supply)
    s = got["summary"]
    print(f"{where}: {want['candidates']} candidates, {want['open']} open, {len(want['absorbed'])} absorbed, {want['matched']} matched, "
          f"{len(want['groups'])} groups, {want['pairs']} pairs")
    assert s["truncated"] == 0, where
    assert (s["candidates"], s["open_emitted"], s["open_stored"]) == (want["candidates"], want["open"], want["open"]), where
    assert s["absorbed_emitted"] == s["absorbed_stored"] == len(want["absorbed"]), where
    assert jx.cells_of(got["absorbed"]) == want["absorbed"], where
    assert jx.product_groups(got) == want["groups"], where
    assert (s["matched"], s["groups"], s["pairs"]) == (want["matched"], len(want["groups"]), want["pairs"]), where
    return want, got


def opposite(groups, a, b):
    """cells a and b lie on opposite sides of one group"""
    return any((a in g[0] and b in g[1]) or (a in g[1] and b in g[0]) for g in groups)


def subset_of_true_groups(got_groups, want_groups):
    for g in got_groups:
        assert g[0] and g[1]
        assert any((set(g[0]) <= set(w[0]) and set(g[1]) <= set(w[1])) or (set(g[0]) <= set(w[1]) and set(g[1]) <= set(w[0])) for w in want_groups), g


# ------------------------------------------------------------------ 1. the join itself
def test_toy_groups_match_the_reference(gpu, toy, toy_all):
    groups = toy_all["groups"]
    # is_real + 1 on a padding row sends three (0): range8.mult + 3 on row 0 receives them; the mirror on the all-zero real row
    assert opposite(groups, (0, PAIRS, 12, IS_REAL, 1), (0, RANGE8, 0, MULT, 3))
    assert opposite(groups, (0, PAIRS, 1, IS_REAL, P - 1), (0, RANGE8, 0, MULT, P - 3))
    # x: 5 -> 6 on row 3 and 6 -> 5 on row 8 (y = z = 0 on both)
    assert opposite(groups, (0, PAIRS, 3, X, 1), (0, PAIRS, 8, X, P - 1))
    check(gpu, [jx.Window(0, toy[c]) for c in (RANGE8, FIB, PAIRS)], DELTAS4, want=toy_all, where="toy, all rows")


def test_the_answer_does_not_depend_on_the_seed(gpu, toy, toy_all):
    ws = [jx.Window(0, toy[c]) for c in (RANGE8, FIB, PAIRS)]
    got = run(gpu, ws, DELTAS4, seed=0xfeedfacecafebeef)
    assert jx.product_groups(got) == toy_all["groups"] and got["summary"]["pairs"] == toy_all["pairs"]


# ------------------------------------------------------------------ 2. absorption
def test_range8_as_supply_absorbs(gpu, toy, toy_supplied):
    soaked = toy_supplied["absorbed"]
    assert (0, PAIRS, 3, X, 1) in soaked                       # x + 1 on a real row with y = 0: (5) -> (6), both in the table
    assert (0, PAIRS, 12, IS_REAL, 1) in soaked                # is_real + 1 on a padding row: three (0)
    assert not any(c[1] == PAIRS and c[3] == X and c[4] == 256 for c in soaked)   # x + 256 is not in the table
    want, got = check(gpu, [jx.Window(0, toy[c]) for c in (FIB, PAIRS)], [1, P - 1, 256], [toy[RANGE8]], want=toy_supplied, where="toy, range8 supplies")
    assert not any(c[1] == RANGE8 for g in jx.product_groups(got) for side in g for c in side)


# ------------------------------------------------------------------ 3. tiny and ragged shapes
SMALL = {0: [(5, 0, 0, 1)], 1: [(5, 0, 0, 1), (6, 0, 0, 1)], 2: [(5, 0, 0, 1), (9, 0, 0, 1), (6, 0, 0, 1)]}


@pytest.mark.parametrize("log_n", [0, 1, 2])
def test_tiny_pairs_tables(gpu, log_n):
    t = pairs_table(log_n, SMALL[log_n])
    want, _ = check(gpu, [jx.Window(0, t)], DELTAS4, where=f"pairs 2^{log_n}")
    if log_n < 2:
        assert not want["groups"]        # every same-table pair is excluded
    else:
        assert opposite(want["groups"], (0, PAIRS, 0, X, 1), (0, PAIRS, 2, X, P - 1))   # rows r and r + 2 may pair


def planted_512():
    """2^9 rows; real rows (5 + (r % 2), 0, 0) up to row 300, so that x + 1 / x - 1 cells are spread over every wave"""
    return pairs_table(9, [(5 + (r % 2), 0, 0, 1) for r in range(300)])


@pytest.mark.parametrize("log_n,first,count", [(4, 3, 11), (9, 0, 65), (9, 100, 257)])
def test_windows(gpu, toy, log_n, first, count):
    t = toy[PAIRS] if log_n == 4 else planted_512()
    check(gpu, [jx.Window(0, t, first, count)], [1, P - 1], where=f"pairs 2^{log_n} rows {first} + {count}")


def test_two_disjoint_windows_of_one_table_are_one_table(gpu):
    """a pair across the windows at row distance 1 stays excluded"""
    t = planted_512()
    ws = [jx.Window(0, t, 0, 64, cols=[X]), jx.Window(0, t, 64, 70, cols=[X])]
    want, _ = check(gpu, ws, [1, P - 1], where="two windows")
    assert want == jx.join([jx.Window(0, t, 0, 134, cols=[X])], [1, P - 1])


# ------------------------------------------------------------------ 4. tags
def test_one_table_under_two_tags(gpu, toy):
    """pairs rows: 0 an all-zero real row, 1 and 3 padding, so is_real - 1 on row 0 cancels is_real + 1 on the rows next to it;
    range8: mult + 1 and mult - 1 on one row cancel.  Under one tag all of these are excluded; across two tags they pair."""
    from dvt_circuits_amd import capi

    t, r8 = pairs_table(2, [(0, 0, 0, 1), (0, 0, 0, 0), (5, 0, 0, 1)]), toy[RANGE8]
    one = jx.join([jx.Window(0, t), jx.Window(0, r8)], [1, P - 1])
    assert not one["groups"] and one["matched"]
    want, _ = check(gpu, [jx.Window(0, t), jx.Window(1, t), jx.Window(0, r8), jx.Window(1, r8)], [1, P - 1], where="tags 0 and 1")
    assert opposite(want["groups"], (0, PAIRS, 0, IS_REAL, P - 1), (1, PAIRS, 1, IS_REAL, 1))      # adjacent rows
    assert opposite(want["groups"], (0, RANGE8, 7, MULT, 1), (1, RANGE8, 7, MULT, P - 1))         # equal rows
    assert want["pairs"] == 256 * (4 - 2) + (2 * 4 - 4)      # of each group's combinations, those under one tag are excluded
    with pytest.raises(capi.DvtError) as e:      # the same rows twice under one tag
        run(gpu, [jx.Window(0, t, 0, 3), jx.Window(0, t, 2, 2)], [1])
    assert e.value.code == capi.DVT_ERR_INPUT and "overlap" in str(e.value)


# ------------------------------------------------------------------ 5. a hot group
def test_hot_group(gpu):
    t = pairs_table(10, [(5, 0, 0, 1)] * 300 + [(6, 0, 0, 1)] * 300)
    want, got = check(gpu, [jx.Window(0, t, cols=[X])], [1, P - 1], where="hot group")
    hot = [g for g in want["groups"] if (0, PAIRS, 0, X, 1) in g[0]]
    assert len(hot) == 1 and len(hot[0][0]) == len(hot[0][1]) == 300
    assert want["pairs"] >= 300 * 300 - 1


# ------------------------------------------------------------------ 6. bounds
def test_record_capacity(gpu, toy, toy_all):
    from dvt_circuits_amd import capi

    ws = [jx.Window(0, toy[c]) for c in (RANGE8, FIB, PAIRS)]
    got = run(gpu, ws, DELTAS4, cap_records=toy_all["open"] - 5)
    s = got["summary"]
    assert s["truncated"] == capi.JOIN_TRUNC_RECORDS
    assert (s["candidates"], s["open_emitted"], s["open_stored"]) == (toy_all["candidates"], toy_all["open"], toy_all["open"] - 5)
    subset_of_true_groups(jx.product_groups(got), toy_all["groups"])


def test_absorbed_capacity(gpu, toy, toy_supplied):
    from dvt_circuits_amd import capi

    n = len(toy_supplied["absorbed"])
    got = run(gpu, [jx.Window(0, toy[c]) for c in (FIB, PAIRS)], [1, P - 1, 256], [toy[RANGE8]], cap_absorbed=n - 3)
    s = got["summary"]
    assert s["truncated"] == capi.JOIN_TRUNC_ABSORBED and (s["absorbed_emitted"], s["absorbed_stored"]) == (n, n - 3)
    assert len(got["absorbed"]) == n - 3 and set(jx.cells_of(got["absorbed"])) <= set(toy_supplied["absorbed"])
    assert jx.product_groups(got) == toy_supplied["groups"] and s["open_emitted"] == toy_supplied["open"]


def test_output_capacity(gpu, toy, toy_all):
    from dvt_circuits_amd import capi

    n_cells = sum(len(side) for g in toy_all["groups"] for side in g)
    got = run(gpu, [jx.Window(0, toy[c]) for c in (RANGE8, FIB, PAIRS)], DELTAS4, cap_cells=n_cells - 1)
    s = got["summary"]
    assert s["truncated"] == capi.JOIN_TRUNC_OUTPUT
    assert (s["open_emitted"], s["matched"], s["groups"], s["pairs"]) == (toy_all["open"], toy_all["matched"], len(toy_all["groups"]), toy_all["pairs"])
    groups = jx.product_groups(got)
    assert sum(len(side) for g in groups for side in g) == n_cells - 1
    for g, w in zip(groups, toy_all["groups"]):
        assert g[0] == w[0][:len(g[0])] and g[1] == w[1][:len(g[1])]


def test_a_join_table_too_small_for_the_differences(gpu, toy, toy_all):
    from dvt_circuits_amd import capi

    assert toy_all["distinct"] > 64          # 2^6 slots cannot hold them: probes must run out
    got = run(gpu, [jx.Window(0, toy[c]) for c in (RANGE8, FIB, PAIRS)], DELTAS4, log_slots=6)
    s = got["summary"]
    assert s["truncated"] == capi.JOIN_TRUNC_PROBES and s["open_emitted"] == toy_all["open"]
    subset_of_true_groups(jx.product_groups(got), toy_all["groups"])


def test_max_evals_one_below_the_need(gpu, toy):
    from dvt_circuits_amd import capi

    w = jx.Window(0, toy[PAIRS])
    need = 4 * 4 * 16 * 2                    # deltas x columns x rows x touched rows
    with pytest.raises(capi.DvtError) as e:
        run(gpu, [w], DELTAS4, max_evals=need - 1)
    assert e.value.code == capi.DVT_ERR_INPUT and "max_evals" in str(e.value)
    assert run(gpu, [w], DELTAS4, max_evals=need)["summary"]["candidates"] == need // 2


def test_a_table_that_is_not_honest_is_rejected(gpu, toy):
    from dvt_circuits_amd import capi

    main = toy[PAIRS].main.copy()
    main[Z, 3] = 1                           # row 3: 5 * 0 != 1
    bad = dict(dev(gpu, toy[PAIRS]), main=internal(gpu, main), tag=0)
    with pytest.raises(capi.DvtError) as e:
        gpu.hunt_join("toy", [bad], [1])
    assert e.value.code == capi.DVT_ERR_REJECTED and "not honest" in str(e.value)


# ------------------------------------------------------------------ the argument checks that need a handle
def test_entries_refuse_bad_arguments(gpu, toy):
    from dvt_circuits_amd import capi

    lib, u32p = gpu.lib, capi.u32p
    t, r8 = dev(gpu, toy[PAIRS]), dev(gpu, toy[RANGE8])
    d = (C.c_uint32 * 1)(1)
    none = (C.c_uint32 * 1)(0)
    h = C.c_void_p()
    assert lib.dvt_stage_hunt_join_new(gpu.h, b"toy", 1, d, 1, 64, 64, 0, C.byref(h)) == capi.DVT_OK
    try:
        add = lambda tag=0, chip=PAIRS, main=t["main"], log_n=4, first=0, count=16, cols=None, n_cols=0: lib.dvt_stage_hunt_join_add(
            gpu.h, h, tag, chip, main.data_ptr() if main is not None else None, None, log_n, none, first, count, cols, n_cols, 0)
        sm = capi.JoinSummary()
        assert lib.dvt_stage_hunt_join_match(gpu.h, h, C.byref(sm)) == capi.DVT_ERR_INPUT          # no window yet
        assert lib.dvt_stage_hunt_join_supply(gpu.h, h, PAIRS, t["main"].data_ptr(), None, 4, none) == capi.DVT_ERR_UNSUPPORTED
        assert lib.dvt_stage_hunt_join_supply(gpu.h, h, 3, t["main"].data_ptr(), None, 4, none) == capi.DVT_ERR_INPUT
        assert lib.dvt_stage_hunt_join_supply(gpu.h, h, RANGE8, None, r8["prep"].data_ptr(), 8, none) == capi.DVT_ERR_INPUT
        bad_col = (C.c_uint32 * 2)(0, 4)
        for what, rc in (("null main", add(main=None)), ("chip", add(chip=3)), ("log_n", add(log_n=23)), ("tag", add(tag=1 << 16)),
                         ("empty window", add(count=0)), ("window past the table", add(first=9, count=8)),
                         ("column", add(cols=bad_col, n_cols=2)), ("empty column list", add(cols=bad_col, n_cols=0))):
            assert rc == capi.DVT_ERR_INPUT, what
        assert add(first=0, count=8) == capi.DVT_OK
        assert add(first=7, count=2) == capi.DVT_ERR_INPUT and "overlap" in lib.dvt_last_error(gpu.h).decode()
        assert add(log_n=3, first=0, count=8, tag=0) == capi.DVT_ERR_INPUT                       # the same instance at another height
        assert lib.dvt_stage_hunt_join_supply(gpu.h, h, RANGE8, r8["main"].data_ptr(), r8["prep"].data_ptr(), 8, none) == capi.DVT_ERR_INPUT
        assert "after the first window" in lib.dvt_last_error(gpu.h).decode()
        n, m = C.c_size_t(), C.c_size_t()
        cell = capi.JoinCell()
        assert lib.dvt_stage_hunt_join_result(gpu.h, h, C.byref(cell), 1, C.byref(n), C.byref(cell), 1, C.byref(m)) == capi.DVT_ERR_INPUT   # before match
        assert add(first=8, count=8) == capi.DVT_OK
        assert lib.dvt_stage_hunt_join_match(gpu.h, h, C.byref(sm)) == capi.DVT_OK and sm.candidates == 64
        assert lib.dvt_stage_hunt_join_match(gpu.h, h, C.byref(sm)) == capi.DVT_ERR_INPUT
        assert add(tag=1) == capi.DVT_ERR_INPUT                                                   # a window after match
    finally:
        assert lib.dvt_stage_hunt_join_free(gpu.h, h) == capi.DVT_OK


# ------------------------------------------------------------------ 7. rv32: cpu and shift windows, three supply tables
PROGRAM, BYTE, CPU, MEM_IMAGE, SHIFT = 0, 1, 2, 3, 5
DELTAS_RV = [1, P - 1, 256, P - 256]


def rv32_tables(elf):
    """{chip id: Table} of a one-shard guest (host-only)"""
    from dvt_circuits_amd import capi

    chips, pubs, n = capi.rv32_debug_traces(elf, [], 21, 0)
    assert n == 1
    return {ch["chip_id"]: hx.Table("rv32", ch["chip_id"], np.ascontiguousarray(ch["main"]), np.ascontiguousarray(ch["prep"]), pubs) for ch in chips}


def window_around(t, column, rows=16):
    """`rows` rows of the table that contain the first row where `column` is set"""
    at = int(np.nonzero(t.main[t.info["desc"].main_names.index(column)])[0][0])
    return max(0, min(at - 4, t.n - rows)), rows


def pair_escapes(tabs, a, b, supply):
    """both changes applied to copies: no unit violated on the touched rows, and the multiset of the union of the touched rows
    unchanged modulo supplied tuples"""
    net = {}
    by_table = {}
    for tag, cid, row, col, delta in (a, b):
        by_table.setdefault((tag, cid), []).append((col, row, delta))
    for (tag, cid), changes in by_table.items():
        t = tabs[cid]
        main = t.main.copy()
        rows = t.touched(changes)
        for col, row, delta in changes:
            main[col, row] = (int(main[col, row]) + delta) % P
        if ex.violated_units(t.machine, cid, main, t.prep, t.pubs, rows=rows):
            return False
        for r in rows:
            for k, v in t.ev.tuples(main, t.prep, t.pubs, r).items():
                net[k] = net.get(k, 0) + v
            for k, v in t._honest_row(r).items():
                net[k] = net.get(k, 0) - v
    return not any(v % P for k, v in net.items() if k not in supply)


@pytest.mark.parametrize("guest", ["arith", "shifts"])
def test_rv32_windows_match_the_reference(gpu, guest):
    from tests import guests

    tabs = rv32_tables(guests.arith(commit=True)[0] if guest == "arith" else guests.shifts()[0])
    cpu = tabs[CPU]
    if guest == "arith":
        windows = [jx.Window(0, cpu, *window_around(cpu, "sys_m"))]       # the first sys row
    else:
        windows = [jx.Window(0, cpu, *window_around(cpu, "is_alu")), jx.Window(0, tabs[SHIFT], 0, 16)]   # a shift instruction; its table rows
    supply = [tabs[PROGRAM], tabs[BYTE], tabs[MEM_IMAGE]]
    want, got = check(gpu, windows, DELTAS_RV, supply, where=f"rv32 {guest}")
    names = {cid: t.info["desc"].main_names for cid, t in tabs.items()}
    show = lambda c: f"{tabs[c[1]].info['name']}.{names[c[1]][c[3]]}@{c[2]}{'+' if c[4] < P // 2 else '-'}{min(c[4], P - c[4])}"
    print("absorbed:", sorted({show(c).split("@")[0] for c in want["absorbed"]}))
    held = jx.supply_set(supply)
    n_pairs = 0
    for g in want["groups"]:
        print("group:", [show(c) for c in g[0]][:6], "x", [show(c) for c in g[1]][:6])
        for a in g[0]:
            for b in g[1]:
                n = tabs[a[1]].n
                if a[:2] == b[:2] and min((a[2] - b[2]) % n, (b[2] - a[2]) % n) <= 1:
                    continue
                n_pairs += 1
                assert pair_escapes(tabs, a, b, held), (show(a), show(b))
    assert n_pairs == want["pairs"]


# ------------------------------------------------------------------ 8. the job-level call
JOB_CFG = '"fri_queries": 6, "pow_bits": 5, "log_shard_size": 12'
JOB_ROWS = 48      # cpu rows per shard: the last of shard 0 and the first of shard 1, either side of the shard boundary


def test_job_call_equals_the_stage_call_and_leaves_the_job_as_found():
    """the cpu tables of both shards of a two-shard job (the cross-shard memory bus), program / byte / mem_image of shard 0
    supplying"""
    from dvt_circuits_amd import capi
    from tests import guests

    elf = guests.commit_only(b"check me")
    p = capi.Prover("{%s}" % JOB_CFG)
    try:
        pk, _ = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 2
        main_w, log_n = p.job_shard_chip_shape(job, 0, CPU)
        assert p.job_shard_chip_shape(job, 1, CPU)[1] >= 6          # (the last shard's table is the shorter one)
        n = 1 << log_n
        windows = [(0, CPU, n - JOB_ROWS, JOB_ROWS), (1, CPU, 0, JOB_ROWS)]
        deltas = [1, P - 1]
        got = p.hunt_join_job(pk, job, windows, deltas)
        print("two-shard job:", got["summary"], [[len(s) for s in g] for g in got["groups"]][:8])
        assert got["summary"]["candidates"] == 2 * JOB_ROWS * main_w * len(deltas) and got["summary"]["truncated"] == 0
        # the stage-level call on the same tables
        shards = [capi.rv32_debug_traces(elf, [], 12, s) for s in (0, 1)]
        assert shards[0][2] == 2
        tab = lambda s, cid: next(hx.Table("rv32", cid, np.ascontiguousarray(ch["main"]), np.ascontiguousarray(ch["prep"]), shards[s][1])
                                  for ch in shards[s][0] if ch["chip_id"] == cid)
        ws = [dict(dev(p, tab(s, CPU)), tag=s, row_first=first, row_count=count) for s, _, first, count in windows]
        want = p.hunt_join("rv32", ws, deltas, supply=[dev(p, tab(0, cid)) for cid in (PROGRAM, BYTE, MEM_IMAGE)])
        assert got == want
        # column lists, and a window to the end of the table
        some = p.hunt_join_job(pk, job, [(0, CPU, n - JOB_ROWS), (1, CPU, 0, JOB_ROWS)], deltas, cols=[[0, 1, 2], None])
        assert some["summary"]["candidates"] == JOB_ROWS * (3 + main_w) * len(deltas)
        for bad in ([(2, CPU, 0, 8)], [(0, 14, 0, 8)], [(0, CPU, n - 4, 8)], []):
            with pytest.raises(capi.DvtError) as e:
                p.hunt_join_job(pk, job, bad, deltas)
            assert e.value.code == capi.DVT_ERR_INPUT, bad
        with pytest.raises(capi.DvtError) as e:
            p.hunt_join_job(pk, job, windows, deltas, supply_chips=(CPU,))
        assert e.value.code == capi.DVT_ERR_UNSUPPORTED
        proof = p.prove_job(pk, job)
        p.job_free(job)
        job2, _ = p.prepare(pk, [])          # never hunted
        assert p.prove_job(pk, job2) == proof
        p.job_free(job2)
        p.pk_free(pk)
    finally:
        p.close()


def test_windows_on_two_members_are_unsupported():
    from dvt_circuits_amd import capi
    from tests import guests

    p = capi.Prover('{%s, "devices": [0, 0]}' % JOB_CFG)
    try:
        pk, _ = p.setup(guests.commit_only(b"check me"))
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 2 and p.job_shard_member(job, 0) != p.job_shard_member(job, 1)
        with pytest.raises(capi.DvtError) as e:
            p.hunt_join_job(pk, job, [(0, CPU, 0, 8), (1, CPU, 0, 8)], [1])
        assert e.value.code == capi.DVT_ERR_UNSUPPORTED
        one = p.hunt_join_job(pk, job, [(1, CPU, 0, 8)], [1])      # on the second member alone it runs
        assert one["summary"]["candidates"] == 8 * 96
        p.job_free(job)
        p.pk_free(pk)
    finally:
        p.close()
