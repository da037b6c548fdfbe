"""GPU tests of the single-cell forgery hunt (hunt.cuh through dvt_stage_hunt_cells): the map of free cells must equal the CPU
reference (tests/_hunt_expect.py: the oracle's generated constraints on the touched rows, and the exact LogUp multiset of the
touched rows) cell by cell.

Toy machine: fib (first, last and transition constraints) at 2^0 (one row is every touched row), 2^1 (row - 1 = row + 1),
2^3 (248 idle lanes that must stay out of the ballots) and 2^9 (two workgroups); pairs and range8 at their own heights.
rv32: every chip on the tables of the small guests, every column, on rows 0, n - 1, the first row with sys_m or is_real set,
the last real row and the first padding row (the three widest chips: row 0, the last real row and the first padding row)."""
import ctypes as C

import numpy as np
import pytest

from tests import _check_expect as ex
from tests import _hunt_expect as hx
from tests import guests, toy_traces
from tests.test_gpu_opening_parity import internal

pytestmark = pytest.mark.gpu
P = hx.P
WIDEST = ("bls_g1", "secp_k1", "fp2_op")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


def toy_table(cid, log_fib=6):
    prep, main, pubs = toy_traces.build(log_fib=log_fib)
    m = dict(main)[cid]
    pr = dict(prep).get(cid)
    return hx.Table("toy", cid, m, pr, pubs if cid == toy_traces.FIB else [])


def device(gpu, t):
    return internal(gpu, t.main), internal(gpu, t.prep) if t.prep.shape[0] else None, t.n.bit_length() - 1


def check_map(gpu, t, deltas, rows, where):
    """the product's map on `rows` (windows of one row, or the whole table when rows is None) against the reference"""
    t_main, t_prep, log_n = device(gpu, t)
    if rows is None:
        counts, fmap = gpu.stage_hunt_cells(t.machine, t.cid, t_main, t_prep, log_n, t.pubs, t.main_w, deltas)
        rows = list(range(t.n))
        assert (counts == fmap.sum(axis=2, dtype=np.uint32).T).all(), where
    else:
        got = []
        for r in rows:
            counts, fm = gpu.stage_hunt_cells(t.machine, t.cid, t_main, t_prep, log_n, t.pubs, t.main_w, deltas, row_first=r, row_count=1)
            assert (counts == fm.sum(axis=2, dtype=np.uint32).T).all(), where
            got.append(fm)
        fmap = np.concatenate(got, axis=2)
    want = t.free_map(deltas, rows)
    bad = np.argwhere(fmap != want)
    print(f"{where}: {int(want.sum())} free of {want.size} (delta, column, row) cells")
    assert bad.size == 0, f"{where}: (delta index, column, row index) {bad[:8].tolist()}: GPU {fmap[tuple(bad[0])]}, reference {want[tuple(bad[0])]}"


@pytest.mark.parametrize("log_fib", [0, 1, 3, 9])
def test_fib_map_matches_the_reference(gpu, log_fib):
    check_map(gpu, toy_table(toy_traces.FIB, log_fib), [1, P - 1, 2], None, f"fib 2^{log_fib}")


@pytest.mark.parametrize("cid", [toy_traces.PAIRS, toy_traces.RANGE8])
def test_pairs_and_range_maps_match_the_reference(gpu, cid):
    check_map(gpu, toy_table(cid), [1, P - 1, 2], None, "pairs" if cid == toy_traces.PAIRS else "range8")


def test_window_agrees_with_the_whole_table(gpu):
    """(5, 70): a partial wave at both ends"""
    t = toy_table(toy_traces.FIB, 9)
    t_main, t_prep, log_n = device(gpu, t)
    deltas = [1, P - 1, 2]
    c_all, m_all = gpu.stage_hunt_cells("toy", t.cid, t_main, t_prep, log_n, t.pubs, 4, deltas, 0, 512)
    c_win, m_win = gpu.stage_hunt_cells("toy", t.cid, t_main, t_prep, log_n, t.pubs, 4, deltas, 5, 70)
    assert m_win.shape == (3, 4, 70) and (m_win == m_all[:, :, 5:75]).all()
    assert (c_win == m_win.sum(axis=2, dtype=np.uint32).T).all() and (c_all == m_all.sum(axis=2, dtype=np.uint32).T).all()
    # the answers for an honest table do not depend on the seed
    assert (gpu.stage_hunt_cells("toy", t.cid, t_main, t_prep, log_n, t.pubs, 4, deltas, 5, 70, seed=0xfeedfacecafebeef)[1] == m_win).all()


# ------------------------------------------------------------------ every rv32 chip
@pytest.fixture(scope="module")
def honest():
    """{chip id: (main, prep, pubs)}: the first table of every chip among the traces of the small guests (host-only)"""
    from dvt_circuits_amd import capi

    elfs = [guests.shifts()[0], guests.muldiv()[0], guests.sha256_precompiled(bytes(range(150)))[0], guests.field_ops()[0],
            guests.curve_ops()[0], guests.u256_ops()[0]]
    tables = {}
    for elf in elfs:
        chips, pubs, n = capi.rv32_debug_traces(elf, [], 21, 0)
        assert n == 1
        for ch in chips:
            tables.setdefault(ch["chip_id"], (np.ascontiguousarray(ch["main"]), np.ascontiguousarray(ch["prep"]), [int(x) for x in pubs]))
    assert sorted(tables) == list(range(14)), "the guests must reach every chip"
    return tables


def rows_of(t):
    names = t.info["desc"].main_names
    n = t.n
    flag = next((names.index(f) for f in ("sys_m", "is_real") if f in names), None)
    real = t.main[names.index("is_real")] if "is_real" in names else sum(t.main[i] for i, nm in enumerate(names) if nm.startswith("is_"))
    n_real = max(1, min(int(np.count_nonzero(real)), n))
    rows = [0, n_real - 1, min(n_real, n - 1)]
    if t.info["name"] not in WIDEST:
        rows.append(n - 1)
        if flag is not None and t.main[flag].any():
            rows.append(int(np.nonzero(t.main[flag])[0][0]))
    return sorted(set(rows))


@pytest.mark.parametrize("cid", range(14))
def test_rv32_chip_map_matches_the_reference(gpu, honest, cid):
    main, prep, pubs = honest[cid]
    t = hx.Table("rv32", cid, main, prep, pubs)
    check_map(gpu, t, [1, P - 1], rows_of(t), f"{t.info['name']} 2^{t.n.bit_length() - 1} rows {rows_of(t)}")


# ------------------------------------------------------------------ the precondition and the argument checks
def raw_cells(gpu, t_main, log_n, pubs, deltas, row_first, row_count, counts, fmap, machine=b"toy", chip=toy_traces.FIB, max_evals=0):
    from dvt_circuits_amd.capi import u32p, u8p

    dl = np.ascontiguousarray(deltas, dtype=np.uint32)
    pv = (C.c_uint32 * 3)(*[int(x) for x in pubs])
    return gpu.lib.dvt_stage_hunt_cells(gpu.h, machine, chip, t_main.data_ptr() if t_main is not None else None, None, log_n, pv, 1,
                                        dl.ctypes.data_as(u32p), dl.size, row_first, row_count, max_evals, counts.ctypes.data_as(u32p),
                                        fmap.ctypes.data_as(u8p))


def test_a_table_that_is_not_honest_is_rejected(gpu):
    from dvt_circuits_amd import capi

    t = toy_table(toy_traces.FIB, 3)
    main = t.main.copy()
    main[2, 4] = (int(main[2, 4]) + 1) % P
    t_main = internal(gpu, main)
    counts, fmap = np.full((4, 1), 0xabababab, np.uint32), np.full((1, 4, 8), 0xab, np.uint8)
    assert raw_cells(gpu, t_main, 3, t.pubs, [1], 0, 8, counts, fmap) == capi.DVT_ERR_REJECTED
    assert "not honest" in gpu.lib.dvt_last_error(gpu.h).decode()
    assert (counts == 0xabababab).all() and (fmap == 0xab).all()
    assert raw_cells(gpu, internal(gpu, t.main), 3, t.pubs, [1], 0, 8, counts, fmap) == capi.DVT_OK
    assert (fmap <= 1).all() and (counts[:, 0] == fmap[0].sum(axis=1)).all()


def test_entry_refuses_bad_arguments(gpu):
    from dvt_circuits_amd import capi

    t = toy_table(toy_traces.FIB, 3)
    t_main = internal(gpu, t.main)
    counts, fmap = np.zeros((4, 8), np.uint32), np.zeros((8, 4, 8), np.uint8)
    ok = dict(t_main=t_main, log_n=3, deltas=[1], row_first=0, row_count=8)
    cases = {"null d_main": dict(t_main=None), "chip out of range": dict(chip=3), "log_n > 22": dict(log_n=23), "no delta": dict(deltas=[]),
             "nine deltas": dict(deltas=list(range(1, 10))), "delta 0": dict(deltas=[1, 0]), "delta p": dict(deltas=[P]),
             "window past the table": dict(row_first=5, row_count=4), "window starts outside": dict(row_first=8, row_count=1),
             "max_evals 1": dict(max_evals=1), "unknown machine": dict(machine=b"nope")}
    for what, change in cases.items():
        assert raw_cells(gpu, pubs=t.pubs, counts=counts, fmap=fmap, **{**ok, **change}) == capi.DVT_ERR_INPUT, what
    assert not counts.any() and not fmap.any()
    # the pair entry: a column at or above main_w, adjacent above 1
    for kw in (dict(cols=[0, 4]), dict(adjacent=2), dict(max_evals=1)):
        with pytest.raises(capi.DvtError) as e:
            gpu.stage_hunt_pairs("toy", toy_traces.FIB, t_main, None, 3, t.pubs, [1], **kw)
        assert e.value.code == capi.DVT_ERR_INPUT, kw
    assert raw_cells(gpu, pubs=t.pubs, counts=counts, fmap=fmap, **ok) == capi.DVT_OK
