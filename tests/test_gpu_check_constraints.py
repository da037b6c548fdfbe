"""GPU tests of check_rows_kernel through dvt_stage_check_constraints: the per-unit violation counts, their sum and the
first (row, unit) must equal what the CPU oracle's generated C constraints give row by row (tests/_check_expect.py), for
every chip of the toy and rv32 machines.

Heights of the random-column cases: 2^0 (one row: the next row is the row itself), 2^3 (the wrap of the next-row rotation
inside a partial block, 248 idle lanes that must not skew the ballots) and 2^9 (two 256-thread blocks).  The honest traces
are those of the small guests of tests/test_gpu_k0_parity.py, which between them reach every chip."""
import numpy as np
import pytest

from tests import _check_expect as ex
from tests import guests
from tests.test_gpu_opening_parity import extreme_words, internal, raw_internal

pytestmark = pytest.mark.gpu
P = 2013265921
MONTY_R = 0x0FFFFFFE   # Montgomery form of 1
SELECTOR_CHIPS = ("cpu", "sha_extend", "sha_compress")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


def columns(gpu, kind, width, n, rng):
    if width == 0:
        return None, np.zeros((0, n), np.uint32)
    if kind == "extreme":
        return raw_internal(gpu, extreme_words(width, n))
    c = rng.integers(0, P, (width, n), dtype=np.uint32)
    return internal(gpu, c), c


def compare(gpu, machine, cid, t_main, t_prep, log_n, pubs, xi, by_row, where):
    info = ex.chip(machine, cid)
    counts, total, row, unit = ex.expectation(machine, cid, by_row)
    gpu.sync()
    r, got = gpu.stage_check_constraints(machine, cid, t_main, t_prep, log_n, pubs, xi, info["nc"])
    print(f"{where}: GPU {r}, oracle violations {total} first ({row}, {unit})")
    bad = np.nonzero(got != counts)[0]
    assert bad.size == 0, f"{where}: counts differ at units {bad[:8].tolist()}: GPU {got[bad[:8]].tolist()}, oracle {counts[bad[:8]].tolist()}"
    assert r["violations"] == total == int(got.astype(np.uint64).sum()), where
    assert (r["first_row"], r["first_constraint"]) == (row, unit), where
    return total


@pytest.mark.parametrize("machine,cid", ex.CHIPS)
def test_random_columns_match_oracle(gpu, machine, cid):
    info = ex.chip(machine, cid)
    rng = np.random.default_rng(4100 + 31 * cid + (machine == "toy"))
    for log_n in (0, 3, 9):
        for kind in ("random", "extreme"):
            n = 1 << log_n
            t_main, main = columns(gpu, kind, info["main_w"], n, rng)
            t_prep, prep = columns(gpu, kind, info["prep_w"], n, rng)
            pubs = rng.integers(0, P, info["n_pub"]).tolist()
            xi = rng.integers(0, P, 4).tolist()
            by_row = ex.violated_units(machine, cid, main, prep, pubs)
            total = compare(gpu, machine, cid, t_main, t_prep, log_n, pubs, xi, by_row, f"{info['name']} 2^{log_n} {kind}")
            if not info["rels"]:   # no identity folded: the oracle's own checker counts the same pairs
                assert total == ex.air(machine).check_constraints(cid, main, prep if info["prep_w"] else np.zeros((1, n), np.uint32), pubs)[0]


def test_entry_refuses_bad_arguments(gpu):
    from dvt_circuits_amd import capi

    t = internal(gpu, np.zeros((4, 8), np.uint32))
    for machine, cid, main in (("toy", 3, t), ("rv32", 14, t), ("toy", 1, None), ("nope", 0, t)):
        with pytest.raises(capi.DvtError) as e:
            gpu.stage_check_constraints(machine, cid, main, None, 3, [0, 0, 0], [1, 2, 3, 4], 7)
        assert e.value.code == capi.DVT_ERR_INPUT
    with pytest.raises(capi.DvtError) as e:
        gpu.stage_check_constraints("toy", 1, t, None, 23, [0, 0, 0], [1, 2, 3, 4], 7)
    assert e.value.code == capi.DVT_ERR_INPUT
    with pytest.raises(capi.DvtError) as e:
        gpu.stage_check_constraints("toy", 1, t, None, 3, [0, 0, 0], [P, 2, 3, 4], 7)
    assert e.value.code == capi.DVT_ERR_INPUT


# ------------------------------------------------------------------ honest rows and single-cell forgeries
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


@pytest.mark.parametrize("cid", range(14))
def test_honest_rows_have_no_violation(gpu, honest, cid):
    """no false positive on padding rows, first / last selectors and the closed-form identities at a real witness"""
    main, prep, pubs = honest[cid]
    info = ex.chip("rv32", cid)
    log_n = main.shape[1].bit_length() - 1
    assert ex.air("rv32").check_constraints(cid, main, prep if info["prep_w"] else np.zeros((1, main.shape[1]), np.uint32), pubs)[0] == 0
    t_main, t_prep = internal(gpu, main), internal(gpu, prep) if info["prep_w"] else None
    xi = np.random.default_rng(77 + cid).integers(0, P, 4).tolist()
    compare(gpu, "rv32", cid, t_main, t_prep, log_n, pubs, xi, {}, f"{info['name']} honest 2^{log_n}")


def forged_cells(info, n, rng):
    """8 (column, row) cells: seeded; row 0 and row n-1 for the chips with first / last / transition constraints; a carry
    column and a quotient column of the first identity for the big-integer chips"""
    cells = [(int(rng.integers(info["main_w"])), int(rng.integers(n))) for _ in range(8)]
    if info["name"] in SELECTOR_CHIPS:
        cells[0] = (cells[0][0], 0)
        cells[1] = (cells[1][0], n - 1)
    if info["name"] in ex.BIG_CHIPS:
        rel = info["desc"].poly_rels[0]
        cells[0] = (rel.w_lo[int(rng.integers(len(rel.w_lo)))].args[1], 0)
        cells[1] = (rel.q[int(rng.integers(len(rel.q)))].args[1], 0)
    return cells


@pytest.mark.parametrize("cid", range(14))
def test_single_cell_forgeries_match_oracle(gpu, honest, cid):
    import torch

    main, prep, pubs = honest[cid]
    info = ex.chip("rv32", cid)
    n = main.shape[1]
    log_n = n.bit_length() - 1
    rng = np.random.default_rng(9000 + cid)
    t_main, t_prep = internal(gpu, main), internal(gpu, prep) if info["prep_w"] else None
    gpu.sync()
    work = main.copy()
    for col, row in forged_cells(info, n, rng):
        work[col, row] = (int(main[col, row]) + 1) % P
        # the rows that read the cell: its own and the one before it (the honest rows violate nothing, checked above)
        by_row = ex.violated_units("rv32", cid, work, prep, pubs, rows=(row - 1, row))
        old = int(t_main[col, row].item())
        t_main[col, row] = (old + MONTY_R) % P
        torch.cuda.synchronize()
        xi = rng.integers(0, P, 4).tolist()
        compare(gpu, "rv32", cid, t_main, t_prep, log_n, pubs, xi, by_row, f"{info['name']} 2^{log_n} cell ({col}, {row}) + 1")
        t_main[col, row] = old
        torch.cuda.synchronize()
        work[col, row] = main[col, row]
