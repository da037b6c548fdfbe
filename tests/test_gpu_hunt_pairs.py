"""GPU tests of the two-cell forgery hunt (hunt.cuh through dvt_stage_hunt_pairs and dvt_rv32_hunt_shard) against the CPU
reference (tests/_hunt_expect.py).

Same-row pairs on the first sys row (COMMIT) of the cpu chip of guests.arith(commit=True): with the cells of the pinned
address expression as columns the reported set must equal the reference's exhaustive one, {(u[0] + 2, u[22] + 1)}; with
every column (164 160 candidates, far beyond the reference's reach) n_tried must be what the free x free rule leaves of the
single-cell map, every report must be an escape for the reference, and 500 seeded candidates that were not reported must be
caught by it.  Adjacent pairs on mem_init of guests.subword() at base rows 0, 700 (the last real row, then the first padding
row) and 1023 (wraps to row 0), and on the toy fib chip at 2^1 and 2^3.  Truncation (cap 0) and the job-level call."""
import numpy as np
import pytest

from tests import _hunt_expect as hx
from tests import guests, toy_traces
from tests.test_gpu_opening_parity import internal

pytestmark = pytest.mark.gpu
P = hx.P
Q, POW = 8, 4
EXPR = ("u[0]", "u[1]", "u[21]", "u[22]", "u[23]")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d}' % (Q, POW))
    yield p
    p.close()


def table_of(elf, name):
    from dvt_circuits_amd import capi

    chips, pubs, n = capi.rv32_debug_traces(elf, [], 21, 0)
    assert n == 1
    cid = next(i for i, c in enumerate(hx.ex.description("rv32").chips) if c.name == name)
    ch = next(c for c in chips if c["chip_id"] == cid)
    return hx.Table("rv32", cid, ch["main"], ch["prep"], pubs)


@pytest.fixture(scope="module")
def cpu():
    """the cpu table, its first sys row, the columns of the address expression, and the table on the device"""
    t = table_of(guests.arith(commit=True)[0], "cpu")
    names = t.info["desc"].main_names
    return dict(t=t, names=names, sys_row=int(np.nonzero(t.main[names.index("sys_m")])[0][0]), cols=[names.index(c) for c in EXPR])


def device(gpu, t):
    return internal(gpu, t.main), internal(gpu, t.prep) if t.prep.shape[0] else None, t.n.bit_length() - 1


def as_tuples(res):
    return [(e["row"], e["col"][0], e["col"][1], e["delta"][0], e["delta"][1], e["alone"]) for e in res["reported"]]


def hunt(gpu, t, dev, deltas, row, **kw):
    res = gpu.stage_hunt_pairs(t.machine, t.cid, dev[0], dev[1], dev[2], t.pubs, deltas, row_first=row, row_count=1, **kw)
    assert res["n_reported"] == len(res["reported"]) and as_tuples(res) == sorted(as_tuples(res))
    assert all(e["n_cells"] == 2 and e["row_off"] == [0, int(bool(kw.get("adjacent")))] for e in res["reported"])
    return res


def test_expression_cells_on_the_sys_row_equal_the_reference(gpu, cpu):
    t, names = cpu["t"], cpu["names"]
    want, tried = t.pairs(hx.DELTAS6, cpu["sys_row"], cpu["cols"])
    res = hunt(gpu, t, device(gpu, t), hx.DELTAS6, cpu["sys_row"], cols=cpu["cols"])
    print("sys row", cpu["sys_row"], "reported", [(names[e[1]], e[3], names[e[2]], e[4], e[5]) for e in as_tuples(res)], "tried", res["n_tried"])
    assert as_tuples(res) == want and res["n_tried"] == tried
    assert want == [(cpu["sys_row"], names.index("u[0]"), names.index("u[22]"), 2, 1, 3)], "the documented freedom of the address expression, and nothing else"
    # truncation: the count stands, nothing is written, no error
    cut = gpu.stage_hunt_pairs("rv32", t.cid, *device(gpu, t), t.pubs, hx.DELTAS6, cols=cpu["cols"], row_first=cpu["sys_row"], row_count=1, cap=0)
    assert cut["n_reported"] == 1 and cut["reported"] == [] and cut["n_tried"] == tried


def test_every_column_on_the_sys_row(gpu, cpu):
    t, row = cpu["t"], cpu["sys_row"]
    dev = device(gpu, t)
    _, fmap = gpu.stage_hunt_cells("rv32", t.cid, dev[0], dev[1], dev[2], t.pubs, t.main_w, hx.DELTAS6, row_first=row, row_count=1)
    fmap = fmap[:, :, 0]
    assert (fmap == t.free_map(hx.DELTAS6, [row])[:, :, 0]).all(), "the map that the expected n_tried and the sample below rest on"
    res = hunt(gpu, t, dev, hx.DELTAS6, row)
    all_pairs = t.main_w * (t.main_w - 1) // 2 * 36
    print(f"sys row {row}: {int(fmap.sum())} free single changes, tried {res['n_tried']} of {all_pairs}, reported {res['n_reported']}")
    assert res["n_tried"] == hx.n_tried_from_map(fmap, fmap, t.main_w, False)
    got = as_tuples(res)
    assert (row, cpu["names"].index("u[0]"), cpu["names"].index("u[22]"), 2, 1, 3) in got
    for r, c0, c1, d0, d1, alone in got:   # each report is an escape for the reference, with the right `alone` bits
        assert c0 < c1 and not t.caught([(c0, r, d0), (c1, r, d1)]), (c0, c1, d0, d1)
        assert alone == (1 if t.caught([(c0, r, d0)]) else 0) | (2 if t.caught([(c1, r, d1)]) else 0) and alone
    # ... and what was not reported (and is not free x free) is caught by the reference
    rng, reported, n = np.random.default_rng(21), {g[1:5] for g in got}, 0
    while n < 500:
        c0, c1 = sorted(int(x) for x in rng.choice(t.main_w, 2, replace=False))
        e0, e1 = (int(x) for x in rng.integers(0, 6, 2))
        d0, d1 = hx.DELTAS6[e0], hx.DELTAS6[e1]
        if (c0, c1, d0, d1) in reported or (fmap[e0, c0] and fmap[e1, c1]):
            continue
        n += 1
        assert t.caught([(c0, row, d0), (c1, row, d1)]), (c0, c1, d0, d1)


def test_adjacent_pairs_of_mem_init(gpu):
    t = table_of(guests.subword()[0], "mem_init")
    names = t.info["desc"].main_names
    n_real = int(np.count_nonzero(t.main[names.index("is_real")]))
    assert (t.main_w, t.n, n_real) == (20, 1024, 701)
    dev = device(gpu, t)
    deltas = [1, P - 1, 256]
    for row in (0, 700, 1023):
        want, tried = t.pairs(deltas, row, adjacent=True)
        res = hunt(gpu, t, dev, deltas, row, adjacent=True)
        print(f"mem_init base row {row}: tried {res['n_tried']}, reported {as_tuples(res)}")
        assert as_tuples(res) == want and res["n_tried"] == tried
        assert want == []


@pytest.mark.parametrize("log_fib", [1, 3])
def test_adjacent_and_same_row_pairs_of_fib(gpu, log_fib):
    prep, main, pubs = toy_traces.build(log_fib=log_fib)
    t = hx.Table("toy", toy_traces.FIB, dict(main)[toy_traces.FIB], None, pubs)
    dev = device(gpu, t)
    deltas = [1, P - 1, 2]
    for adjacent in (True, False):
        res = gpu.stage_hunt_pairs("toy", t.cid, dev[0], dev[1], dev[2], t.pubs, deltas, adjacent=adjacent)
        want, tried = [], 0
        for row in range(t.n):
            w, k = t.pairs(deltas, row, adjacent=adjacent)
            want, tried = want + w, tried + k
        print(f"fib 2^{log_fib} adjacent={adjacent}: tried {res['n_tried']}, reported {res['n_reported']}")
        assert as_tuples(res) == sorted(want) and res["n_tried"] == tried and res["n_reported"] == len(want)


def test_hunt_shard_equals_the_stage_calls_and_leaves_the_job_as_found(gpu, cpu):
    from dvt_circuits_amd import capi

    elf = guests.arith(commit=True)[0]
    t, row = cpu["t"], cpu["sys_row"]
    log_n = t.n.bit_length() - 1
    pk, vk = gpu.setup(elf)
    job, _ = gpu.prepare(pk, [])
    assert gpu.job_shards(job) == 1 and gpu.job_shard_chip_shape(job, 0, t.cid) == (t.main_w, log_n)
    counts, fmap = gpu.hunt_shard(pk, job, 0, t.cid, hx.DELTAS6, row_first=row, row_count=1)
    pairs = gpu.hunt_shard(pk, job, 0, t.cid, hx.DELTAS6, pairs=True, cols=cpu["cols"], row_first=row, row_count=1)
    with pytest.raises(capi.DvtError) as e:   # a shard the job does not hold
        gpu.hunt_shard(pk, job, 1, t.cid, hx.DELTAS6, row_first=row, row_count=1)
    assert e.value.code == capi.DVT_ERR_INPUT
    proof = gpu.prove_job(pk, job)
    # the stage calls on the device's own traces of that shard
    chips, pubs = gpu.debug_device_traces(pk, job, 0)
    main = next(c for c in chips if c["chip_id"] == t.cid)["main"]
    assert main.shape == t.main.shape and [int(x) for x in pubs] == t.pubs
    t_main, t_prep = internal(gpu, np.ascontiguousarray(main)), internal(gpu, t.prep) if t.prep.shape[0] else None
    s_counts, s_fmap = gpu.stage_hunt_cells("rv32", t.cid, t_main, t_prep, log_n, t.pubs, t.main_w, hx.DELTAS6, row_first=row, row_count=1)
    s_pairs = gpu.stage_hunt_pairs("rv32", t.cid, t_main, t_prep, log_n, t.pubs, hx.DELTAS6, cols=cpu["cols"], row_first=row, row_count=1)
    assert (counts == s_counts).all() and (fmap == s_fmap).all() and pairs == s_pairs and pairs["n_reported"] == 1
    gpu.job_free(job)
    # a job that was never hunted proves to the same bytes
    job2, _ = gpu.prepare(pk, [])
    assert gpu.prove_job(pk, job2) == proof
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok, why
    gpu.job_free(job2)
    gpu.pk_free(pk)
