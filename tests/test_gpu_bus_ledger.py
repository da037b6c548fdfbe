"""GPU tests of the bus ledger (ledger_rows_kernel in its TALLY and COLLECT modes, the close kernel, the record table)
through dvt_stage_bus_ledger_* and dvt_rv32_job_bus_tuples.

The yardstick everywhere is the oracle's exact multiset over the same canonical matrices (tests/_orc.py).  Two conditions:
the GPU names as many tuples as the oracle counts unbalanced, and handing every GPU tuple back to the oracle as a receive of
its net multiplicity balances the oracle's multiset to 0.  Together: the GPU's set IS the oracle's set, nets included.

2^3 rows: a partial wave, everything unmatched, every tuple's bucket dirty; 2^9 rows: two blocks, with the LogUp groups of
cpu (4), muldiv (2) and bls_g1 (16) on grid.y.  The sparse cases run on the three-shard job of tests/test_gpu_bus_sums.py.

The multiplicity-off-by-one case: the tuple is received once by the byte table of EVERY shard that looks it up, so n_recv is
the number of byte tables with a non-zero multiplicity of that row (counted from the oracle's interactions), which is 1 only
when a single shard uses the row."""
import ctypes as C

import numpy as np
import pytest

from tests import _check_expect as ex
from tests import guests
from tests.test_gpu_check_constraints import columns
from tests.test_gpu_opening_parity import internal
from tests.test_rv32_exec_trace import pv_extra

pytestmark = pytest.mark.gpu
P = 2013265921
Q, POW = 8, 4
CFG = '"fri_queries": %d, "pow_bits": %d' % (Q, POW)
PV = b"check me"
u32p = C.POINTER(C.c_uint32)
INTER_FN = C.CFUNCTYPE(None, u32p, u32p, u32p, u32p, u32p, u32p, u32p)
TWO_BLOCK_CHIPS = ("cpu", "muldiv", "bls_g1")


class InterInfo(C.Structure):
    _fields_ = [("bus", C.c_int32), ("sign", C.c_int32), ("scope", C.c_int32), ("arity", C.c_int32)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


# ------------------------------------------------------------------ the oracle's side
def occurrences(machine, cid, main, prep, pubs):
    """the oracle's generated `interactions` on every row: (info [ni] of (bus, sign, arity), mult [n][ni], vals [n][ni][A])"""
    ch = ex.air(machine).chip(cid)
    ni, A, n = ch.n_interactions, max(ch.max_arity, 1), main.shape[1]
    info = [(i.bus, i.sign, i.arity) for i in C.cast(ch.inter, C.POINTER(InterInfo))[:ni]]
    mult, vals = np.zeros((n, max(ni, 1)), np.uint32), np.zeros((n, max(ni, 1), A), np.uint32)
    if not ni:
        return info, mult, vals
    fn = INTER_FN(ch.interactions)
    pad = lambda v: np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint32).ravel(), np.zeros(1, np.uint32)]))
    pub = pad(pubs)
    for r in range(n):
        rn = (r + 1) % n
        ml, mn, pl, pn = pad(main[:, r]), pad(main[:, rn]), pad(prep[:, r]), pad(prep[:, rn])
        fn(*[a.ctypes.data_as(u32p) for a in (ml, mn, pl, pn, pub, mult[r], vals[r])])
    return info, mult, vals


def where_it_occurs(occ, t):
    """[(row, interaction, sign)] of the tuple t among the occurrences of a table, in the ledger's order"""
    info, mult, vals = occ
    out = []
    for j, (bus, sign, arity) in enumerate(info):
        if bus != t["bus"] or arity != t["arity"]:
            continue
        hit = (vals[:, j, :arity] == np.asarray(t["values"], np.uint32)).all(axis=1) & (mult[:, j] != 0)
        out += [(int(r), j, sign) for r in np.nonzero(hit)[0]]
    return sorted(out)


def is_the_oracles_set(groups, extra, tuples, where, machine="rv32"):
    """the two conditions of the module docstring; returns the oracle's count"""
    air, clean = ex.air(machine), groups
    n_oracle, first = air.logup_unbalanced(clean, extra=list(extra))
    print(f"{where}: GPU names {len(tuples)} tuples, the oracle counts {n_oracle} (its first: {first})")
    assert len(tuples) == n_oracle, where
    assert all(0 < t["net"] < P for t in tuples), where
    back = list(extra) + [(t["bus"], t["values"], -1, t["net"]) for t in tuples]
    left, first = air.logup_unbalanced(clean, extra=back)
    assert left == 0, f"{where}: {left} tuples stay unbalanced after the GPU's tuples are handed back, first {first}"
    return n_oracle


def run_ledger(p, machine, tables, extra=(), log_buckets=20, cap_slots=1 << 16, seed=0x5EED, cap=1 << 16):
    """tables: (chip, t_main, t_prep, log_n, pubs, tag).  TALLY, close, COLLECT over the same, result: (n_dirty, tuples, truncated)"""
    L = p.bus_ledger(machine, log_buckets, cap_slots, seed)
    try:
        for t in tables:
            L.add(*t)
        for bus, vals, sign, mult in extra:
            L.add_tuple(bus, vals, sign, mult)
        n_dirty = L.close()
        for t in tables:
            L.collect(*t)
        for bus, vals, sign, mult in extra:
            L.add_tuple(bus, vals, sign, mult)
        tuples, truncated = L.result(cap)
    finally:
        L.free()
    return n_dirty, tuples, truncated


def ordered(tuples):
    return sorted(tuples, key=lambda t: (t["bus"], t["values"])) == tuples


# ------------------------------------------------------------------ every chip, random and extreme columns
@pytest.mark.parametrize("machine,cid", ex.CHIPS)
def test_every_chip_matches_the_oracle_multiset(gpu, machine, cid):
    info = ex.chip(machine, cid)
    rng = np.random.default_rng(7300 + 17 * cid + (machine == "toy"))
    for log_n in (3, 9) if info["name"] in TWO_BLOCK_CHIPS else (3,):
        for kind in ("random", "extreme"):
            n = 1 << log_n
            t_main, main = columns(gpu, kind, info["main_w"], n, rng)
            t_prep, prep = columns(gpu, kind, info["prep_w"], n, rng)
            pubs = rng.integers(0, P, info["n_pub"]).tolist()
            gpu.sync()
            tag = int(rng.integers(1 << 16))
            big = info["ni"] * n > 1 << 15
            n_dirty, tuples, truncated = run_ledger(gpu, machine, [(cid, t_main, t_prep, log_n, pubs, tag)],
                                                    cap_slots=1 << 20 if big else 1 << 16, cap=1 << 19 if big else 1 << 16)
            where = f"{info['name']} 2^{log_n} {kind}"
            assert not truncated and ordered(tuples), where
            oracle_prep = prep if info["prep_w"] else np.zeros((1, n), np.uint32)
            group = [([dict(chip_id=cid, main=main, prep=oracle_prep)], pubs)]
            n_oracle = is_the_oracles_set(group, (), tuples, where, machine)
            assert (n_dirty > 0) == (n_oracle > 0) and n_dirty <= n_oracle, where
            if kind == "random" and info["ni"]:
                assert n_oracle > 0, f"{where}: random columns must leave tuples unmatched"
            # the lowest occurrence and the counters of three tuples, from the oracle's interactions on the rows
            occ = occurrences(machine, cid, main, oracle_prep, pubs)
            for k in sorted(set(int(x) for x in rng.integers(0, max(len(tuples), 1), 3))) if tuples else []:
                t = tuples[k]
                at = where_it_occurs(occ, t)
                assert at, f"{where}: tuple {k} occurs on no row"
                assert (t["first_tag"], t["first_chip"], t["first_row"], t["first_interaction"]) == (tag, cid, at[0][0], at[0][1]), (where, t, at[:3])
                assert (t["n_send"], t["n_recv"]) == (sum(s > 0 for _, _, s in at), sum(s <= 0 for _, _, s in at)), (where, t)


# ------------------------------------------------------------------ truncation and order errors
def test_a_full_record_table_truncates_but_stays_exact(gpu):
    info = ex.chip("rv32", 2)
    rng = np.random.default_rng(7411)
    t_main, main = columns(gpu, "random", info["main_w"], 8, rng)
    t_prep, prep = columns(gpu, "random", info["prep_w"], 8, rng)
    pubs = rng.integers(0, P, info["n_pub"]).tolist()
    gpu.sync()
    n_dirty, tuples, truncated = run_ledger(gpu, "rv32", [(2, t_main, t_prep, 3, pubs, 0)], cap_slots=16)
    air = ex.air("rv32")
    group = [([dict(chip_id=2, main=main, prep=prep if info["prep_w"] else np.zeros((1, 8), np.uint32))], pubs)]
    n_oracle, _ = air.logup_unbalanced(group)
    print(f"cap_slots 16: {len(tuples)} tuples of the oracle's {n_oracle}, truncated {truncated}")
    assert n_oracle > 16 and truncated and 0 < len(tuples) <= 16
    # each returned tuple is unmatched in the oracle with the oracle's net: handing them back clears exactly that many
    left, _ = air.logup_unbalanced(group, extra=[(t["bus"], t["values"], -1, t["net"]) for t in tuples])
    assert left == n_oracle - len(tuples)
    # the caller's array too small: the first tuples of the sorted list, and truncated
    n_dirty, few, truncated = run_ledger(gpu, "rv32", [(2, t_main, t_prep, 3, pubs, 0)], cap=5)
    _, every, whole = run_ledger(gpu, "rv32", [(2, t_main, t_prep, 3, pubs, 0)])
    assert truncated and not whole and len(every) == n_oracle and few == every[:5]


def test_wrong_order_is_refused_and_the_handle_keeps_working(gpu):
    from dvt_circuits_amd import capi

    info = ex.chip("toy", 2)
    rng = np.random.default_rng(7412)
    t_main, main = columns(gpu, "random", info["main_w"], 8, rng)
    gpu.sync()
    L = gpu.bus_ledger("toy", 10, 64, 3)
    with pytest.raises(capi.DvtError) as e:
        L.collect(2, t_main, None, 3, [], 0)
    assert e.value.code == capi.DVT_ERR_INPUT
    L.add(2, t_main, None, 3, [], 0)
    for bad in (dict(chip=3), dict(log_n=23), dict(tag=1 << 16)):
        with pytest.raises(capi.DvtError) as e:
            L.add(bad.get("chip", 2), t_main, None, bad.get("log_n", 3), [], bad.get("tag", 0))
        assert e.value.code == capi.DVT_ERR_INPUT
    with pytest.raises(capi.DvtError) as e:
        L.add_tuple(1, [0] * 41, 1, 1)
    assert e.value.code == capi.DVT_ERR_INPUT
    assert L.close() > 0
    with pytest.raises(capi.DvtError) as e:
        L.add(2, t_main, None, 3, [], 0)
    assert e.value.code == capi.DVT_ERR_INPUT
    L.collect(2, t_main, None, 3, [], 0)
    tuples, truncated = L.result()
    L.free()
    group = [([dict(chip_id=2, main=main, prep=np.zeros((1, 8), np.uint32))], [])]
    is_the_oracles_set(group, (), tuples, "toy pairs after refused calls", "toy")
    assert not truncated


# ------------------------------------------------------------------ the three-shard job: sparse cases
@pytest.fixture(scope="module")
def job3():
    """the three-shard commit_only job at 2^11 cycles per shard: its device traces (canonical) with the preprocessed
    columns of the host traces, and every table on the device"""
    from dvt_circuits_amd import capi

    p = capi.Prover('{%s, "log_shard_size": 11}' % CFG)
    elf = guests.commit_only(PV)
    pk, vk = p.setup(elf)
    job, _ = p.prepare(pk, [])
    assert p.job_shards(job) == 3
    shards = []
    for s in range(3):
        dev, pubs = p.debug_device_traces(pk, job, s)
        host, _, _ = capi.rv32_debug_traces(elf, [], 11, s)
        assert [c["chip_id"] for c in host] == [c["chip_id"] for c in dev]
        shards.append(([dict(chip_id=d["chip_id"], main=np.ascontiguousarray(d["main"]), prep=np.ascontiguousarray(h["prep"])) for d, h in zip(dev, host)],
                       [int(x) for x in pubs]))
    tables = {}
    for s, (chips, pubs) in enumerate(shards):
        for ch in chips:
            has_prep = ex.chip("rv32", ch["chip_id"])["prep_w"]
            tables[s, ch["chip_id"]] = (ch["chip_id"], internal(p, ch["main"]), internal(p, ch["prep"]) if has_prep else None,
                                        ch["main"].shape[1].bit_length() - 1, pubs, s)
    p.sync()
    yield dict(p=p, elf=elf, pk=pk, vk=vk, job=job, shards=shards, tables=tables, extra=pv_extra(PV))
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def with_table(j, shard, cid, main):
    """(the oracle's groups, the ledger's tables) with one main matrix replaced"""
    groups = [([dict(c, main=main) if (s, c["chip_id"]) == (shard, cid) else c for c in chips], pubs) for s, (chips, pubs) in enumerate(j["shards"])]
    tables = dict(j["tables"])
    old = tables[shard, cid]
    tables[shard, cid] = (old[0], internal(j["p"], main)) + old[2:]
    j["p"].sync()
    return groups, list(tables.values())


def test_honest_traces_leave_every_bucket_clean(job3):
    n_dirty, tuples, truncated = run_ledger(job3["p"], "rv32", list(job3["tables"].values()), job3["extra"])
    assert (n_dirty, tuples, truncated) == (0, [], False)
    # without the verifier's side the eight COMMIT sends are what does not cancel
    n_dirty, tuples, truncated = run_ledger(job3["p"], "rv32", list(job3["tables"].values()))
    is_the_oracles_set(job3["shards"], (), tuples, "honest traces without the verifier's tuples")
    assert len(tuples) == 8 and all(t["bus"] == 5 and t["n_send"] == 1 and t["n_recv"] == 0 for t in tuples)


def test_a_forged_memory_value_names_its_tuples(job3):
    air = ex.air("rv32")
    col = ex.chip("rv32", 2)["desc"].main_names.index("b[0]")
    cpu = next(c for c in job3["shards"][1][0] if c["chip_id"] == 2)
    for row in range(5, 13):
        forged = cpu["main"].copy()
        forged[col, row] = (int(forged[col, row]) + 1) % P
        groups, tables = with_table(job3, 1, 2, forged)
        if air.logup_unbalanced(groups, extra=job3["extra"])[0]:
            break
    else:
        pytest.fail("forging b[0] changes no tuple on rows 5..12")
    n_dirty, tuples, truncated = run_ledger(job3["p"], "rv32", tables, job3["extra"])
    assert n_dirty and not truncated and ordered(tuples)
    is_the_oracles_set(groups, job3["extra"], tuples, f"b[0] of row {row} forged")
    # every tuple occurs on the forged row of shard 1's cpu table, or is the partner that lost its match (the honest row's)
    pubs = job3["shards"][1][1]
    occ_forged, occ_honest = occurrences("rv32", 2, forged, cpu["prep"], pubs), occurrences("rv32", 2, cpu["main"], cpu["prep"], pubs)
    for t in tuples:
        here = [r for r, _, _ in where_it_occurs(occ_forged, t) if r in (row - 1, row)]
        partner = [r for r, _, _ in where_it_occurs(occ_honest, t) if r in (row - 1, row)]
        assert here or partner, t


def test_a_multiplicity_off_by_one_is_one_tuple_on_a_hot_record(job3):
    air = ex.air("rv32")
    byte = next(c for c in job3["shards"][0][0] if c["chip_id"] == 1)
    col, row = np.unravel_index(int(np.argmax(byte["main"])), byte["main"].shape)
    forged = byte["main"].copy()
    forged[col, row] = (int(forged[col, row]) + 1) % P
    groups, tables = with_table(job3, 0, 1, forged)
    n_oracle, first = air.logup_unbalanced(groups, extra=job3["extra"])
    assert n_oracle == 1
    n_dirty, tuples, truncated = run_ledger(job3["p"], "rv32", tables, job3["extra"])
    is_the_oracles_set(groups, job3["extra"], tuples, f"byte multiplicity ({col}, {row}) + 1")
    assert n_dirty == 1 and len(tuples) == 1 and not truncated
    t = tuples[0]
    assert [t["bus"], t["arity"], t["net"]] + t["values"] == first
    sends = receives = 0
    for chips, pubs in groups:
        for ch in chips:
            at = where_it_occurs(occurrences("rv32", ch["chip_id"], ch["main"], ch["prep"], pubs), t)
            sends += sum(s > 0 for _, _, s in at)
            receives += sum(s <= 0 for _, _, s in at)
    print(f"byte row {row} column {col} multiplicity {int(byte['main'][col, row])} + 1: tuple {t}, oracle sends {sends} receives {receives}")
    assert t["n_send"] == sends and sends > 0
    assert t["n_recv"] == receives and 1 <= receives <= 3   # one per byte table that holds the row with a multiplicity
    assert (t["first_tag"], t["first_chip"], t["first_row"]) == (0, 1, row)


# ------------------------------------------------------------------ job level
def test_whole_job_has_no_tuple_and_proves_the_same_bytes():
    from dvt_circuits_amd import capi

    proofs = []
    for ledger in (True, False):
        p = capi.Prover('{%s, "log_shard_size": 11}' % CFG)
        pk, vk = p.setup(guests.commit_only(PV))
        job, _ = p.prepare(pk, [])
        if ledger:
            assert p.job_bus_tuples(pk, job) == ([], False)
        proofs.append(p.prove_job(pk, job))
        if ledger:   # phase 1 consumed: K0 runs again
            assert p.job_bus_tuples(pk, job) == ([], False)
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, _, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == PV, why


def partial_tuples(cfg_extra):
    from dvt_circuits_amd import capi

    p = capi.Prover('{%s, "log_shard_size": 11%s}' % (CFG, cfg_extra))
    pk, _ = p.setup(guests.commit_only(PV))
    job, _ = p.prepare(pk, [], first=0, stride=2)
    assert p.job_shards(job) == 3
    out = p.job_bus_tuples(pk, job)
    p.job_free(job)
    p.pk_free(pk)
    p.close()
    return out


def test_partial_job_names_what_does_not_cancel_among_its_shards(job3):
    tuples, truncated = partial_tuples("")
    assert tuples and not truncated and ordered(tuples)
    groups = [job3["shards"][0], job3["shards"][2]]
    is_the_oracles_set(groups, job3["extra"], tuples, "shards 0 and 2 of 3")
    assert {t["first_tag"] for t in tuples} <= {0, 2}
    two, truncated = partial_tuples(', "devices": [0, 0]')
    assert not truncated and two == tuples
