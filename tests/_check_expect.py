"""What dvt_stage_check_constraints must report for a trace, from the CPU oracle alone (test infrastructure).

The generated C `constraints` function of orc_chip_air is called row by row through ctypes; the `when` predicate of
oracle/air_oracle.c (all rows, row 0, row n-1, every row but the last) is applied; the coefficient constraints first ..
first + K - 1 of every big-integer identity are folded onto `first` (the unit the product reports).  The (first, K) pairs
come from the machine description (tools/airgen, poly_rels)."""
import ctypes as C
import functools
import importlib

import numpy as np

from tests import _orc

u32p = C.POINTER(C.c_uint32)
ROW_FN = C.CFUNCTYPE(None, u32p, u32p, u32p, u32p, u32p, u32p)
MACHINES = ("toy", "rv32")
CHIPS = [("toy", c) for c in range(3)] + [("rv32", c) for c in range(14)]
BIG_CHIPS = ("fp_op", "fp2_op", "bls_g1", "secp_k1", "u256_mul")


@functools.lru_cache(maxsize=None)
def description(machine):
    return importlib.import_module(f"tools.airgen.{machine}").build()


@functools.lru_cache(maxsize=None)
def air(machine):
    return _orc.air(machine)


@functools.lru_cache(maxsize=None)
def chip(machine, cid):
    """sizes of the chip, its row function, its `when` codes and the unit of every constraint index"""
    ch = air(machine).chip(cid)
    desc = description(machine).chips[cid]
    assert desc.name == ch.name.decode() and len(desc.constraints) == ch.n_constraints
    unit = np.arange(ch.n_constraints)
    rels = [(r.first, r.K) for r in getattr(desc, "poly_rels", [])]
    for first, k in rels:
        unit[first:first + k] = first
    when = np.ctypeslib.as_array((C.c_uint8 * max(ch.n_constraints, 1)).from_address(ch.when or 0))[:ch.n_constraints].copy() if ch.n_constraints else np.zeros(0, np.uint8)
    buses = sorted({description(machine).buses[i.bus] for i in desc.interactions})
    return dict(name=desc.name, main_w=ch.main_w, prep_w=ch.prep_w, n_pub=ch.n_pub, nc=ch.n_constraints, ni=ch.n_interactions,
                fn=ROW_FN(ch.constraints) if ch.n_constraints else None, when=when, unit=unit, rels=rels, buses=buses, desc=desc)


def violated_units(machine, cid, main, prep, pubs, rows=None):
    """{row: sorted units violated on that row} for the given rows (default: all) of canonical column-major matrices"""
    info = chip(machine, cid)
    n = main.shape[1]
    if not info["nc"]:
        return {}
    pad = lambda v: np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint32).ravel(), np.zeros(1, np.uint32)]))
    pub = pad(pubs)
    out = np.zeros(info["nc"] + 1, np.uint32)
    when, unit = info["when"], info["unit"]
    res = {}
    for r in (range(n) if rows is None else sorted(set(int(x) % n for x in rows))):
        rn = (r + 1) % n
        ml, mn, pl, pn = pad(main[:, r]), pad(main[:, rn]), pad(prep[:, r]), pad(prep[:, rn])
        info["fn"](*[a.ctypes.data_as(u32p) for a in (ml, mn, pl, pn, pub, out)])
        active = (when == 0) | ((when == 1) & (r == 0)) | ((when == 2) & (r == n - 1)) | ((when == 3) & (r != n - 1))
        bad = np.nonzero(active & (out[:info["nc"]] != 0))[0]
        if bad.size:
            res[r] = sorted(set(unit[bad].tolist()))
    return res


def expectation(machine, cid, by_row):
    """(counts [n_constraints], violations, first_row, first_constraint) as the product reports them"""
    counts = np.zeros(chip(machine, cid)["nc"], np.uint32)
    for units in by_row.values():
        counts[units] += 1
    if not by_row:
        return counts, 0, 0, -1
    r0 = min(by_row)
    return counts, int(counts.sum()), r0, by_row[r0][0]
