"""GPU tests of bus_rows_kernel + bus_fold_kernel through dvt_stage_bus_sums: the per-bus sums of a chip's signed LogUp
terms.  Their sum over the buses must equal, word for word, the cumulative sum of the oracle's K4 restatement
(orc_perm_trace) at the same challenges, and a bus the chip's interaction table does not name must stay exactly zero.
2^3 rows: a partial block; 2^9 rows: two blocks, and the LogUp groups of the part-parallel chips on grid.y.

On the honest traces of a three-shard job the sums over all chips and shards vanish on every bus but `sys` (whose
receiving side the verifier supplies); a forged memory-value cell of the cpu chip unbalances the bus the oracle's exact
multiset names."""
import numpy as np
import pytest

from tests import _check_expect as ex
from tests import guests
from tests.test_gpu_check_constraints import columns
from tests.test_gpu_opening_parity import internal

pytestmark = pytest.mark.gpu
P = 2013265921
SYS_BUS = 5          # tools/airgen/rv32.py BUSES["sys"]
CFG = '"fri_queries": 8, "pow_bits": 4'


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


def add_words(a, b):
    return ((a.astype(np.uint64) + b.astype(np.uint64)) % P).astype(np.uint32)


@pytest.mark.parametrize("machine,cid", ex.CHIPS)
def test_bus_sums_add_up_to_the_oracle_cumulative_sum(gpu, machine, cid):
    info = ex.chip(machine, cid)
    rng = np.random.default_rng(5200 + 13 * cid + (machine == "toy"))
    for log_n in (3, 9):
        for kind in ("random", "extreme"):
            n = 1 << log_n
            t_main, main = columns(gpu, kind, info["main_w"], n, rng)
            t_prep, prep = columns(gpu, kind, info["prep_w"], n, rng)
            pubs = rng.integers(0, P, info["n_pub"]).tolist()
            alpha, beta = rng.integers(0, P, 4).tolist(), rng.integers(0, P, 4).tolist()
            _, want = ex.air(machine).perm_trace(cid, main, prep if info["prep_w"] else np.zeros((1, n), np.uint32), pubs, alpha, beta)
            gpu.sync()
            out = gpu.stage_bus_sums(machine, cid, t_main, t_prep, log_n, pubs, alpha, beta)
            where = f"{info['name']} 2^{log_n} {kind}"
            assert (out < P).all(), where
            total = np.zeros(4, np.uint32)
            for b in range(out.shape[0]):
                total = add_words(total, out[b])
                if b not in info["buses"]:
                    assert not out[b].any(), f"{where}: bus {b} is not in the chip's interaction table but sums to {out[b].tolist()}"
            print(f"{where}: GPU sum over buses {total.tolist()}, oracle cumulative sum {want.tolist()}")
            assert total.tolist() == want.tolist(), where
            assert any(out[b].any() for b in info["buses"]), f"{where}: every bus of the chip sums to zero on random columns"


def three_shard_job(p):
    from dvt_circuits_amd import capi  # noqa: F401

    elf = guests.commit_only(b"check me")
    pk, vk = p.setup(elf)
    job, _ = p.prepare(pk, [])
    return elf, pk, job


def test_shard_traces_balance_on_every_bus_but_sys(gpu):
    import torch
    from dvt_circuits_amd import capi

    p = capi.Prover('{%s, "log_shard_size": 11}' % CFG)
    elf, pk, job = three_shard_job(p)
    n_shards = p.job_shards(job)
    assert n_shards == 3
    rng = np.random.default_rng(61)
    alpha, beta = rng.integers(0, P, 4).tolist(), rng.integers(0, P, 4).tolist()
    shards = []
    for s in range(n_shards):
        dev, pubs = p.debug_device_traces(pk, job, s)
        host, hpubs, _ = capi.rv32_debug_traces(elf, [], 11, s)     # (for the preprocessed columns)
        assert [c["chip_id"] for c in host] == [c["chip_id"] for c in dev]
        shards.append(([dict(chip_id=d["chip_id"], main=np.ascontiguousarray(d["main"]), prep=np.ascontiguousarray(h["prep"])) for d, h in zip(dev, host)],
                       [int(x) for x in pubs]))

    def sums(forge=None):
        total = np.zeros((capi.CHECK_BUSES, 4), np.uint32)
        for s, (chips, pubs) in enumerate(shards):
            for ch in chips:
                info = ex.chip("rv32", ch["chip_id"])
                main = ch["main"]
                if forge and forge[:2] == (s, ch["chip_id"]):
                    main = main.copy()
                    main[forge[2], forge[3]] = (int(main[forge[2], forge[3]]) + 1) % P
                t_main, t_prep = internal(p, main), internal(p, ch["prep"]) if info["prep_w"] else None
                p.sync()
                out = p.stage_bus_sums("rv32", ch["chip_id"], t_main, t_prep, main.shape[1].bit_length() - 1, pubs, alpha, beta)
                for b in range(capi.CHECK_BUSES):
                    total[b] = add_words(total[b], out[b])
        return total

    total = sums()
    print("honest sums per bus:", total.tolist())
    for b in range(capi.CHECK_BUSES):
        assert b == SYS_BUS or not total[b].any(), f"bus {b} does not balance on honest traces: {total[b].tolist()}"
    assert total[SYS_BUS].any(), "the sys bus carries the COMMIT tuples, whose receiving side is the verifier's"

    # one cell of a memory-value column of the cpu chip (b: the word read from register rs1, a tuple of the mem bus), on the
    # first row from 5 on where the oracle's exact multiset sees the forgery
    names = ex.chip("rv32", 2)["desc"].main_names
    col = names.index("b[0]")
    cpu = next(c for c in shards[1][0] if c["chip_id"] == 2)
    honest_total = total
    from tests.test_rv32_exec_trace import pv_extra   # the verifier's receiving side of the COMMIT tuples on the sys bus

    extra = pv_extra(b"check me")
    assert ex.air("rv32").logup_unbalanced(shards, extra=extra)[0] == 0, "the honest shard traces must balance exactly"
    for row in range(5, 13):
        forged = [dict(c) for c in shards[1][0]]
        for c in forged:
            if c["chip_id"] == 2:
                c["main"] = c["main"].copy()
                c["main"][col, row] = (int(cpu["main"][col, row]) + 1) % P
        n_bad, first = ex.air("rv32").logup_unbalanced([shards[0], (forged, shards[1][1]), shards[2]], extra=extra)
        if n_bad:
            break
    assert n_bad and first is not None, f"forging column {names[col]} changes no tuple on rows 5..12"
    bad_bus = int(first[0])
    total = sums(forge=(1, 2, col, row))
    # (non-zero, or for the sys bus: no longer the verifier-side term the honest traces add up to)
    nonzero = [b for b in range(capi.CHECK_BUSES) if (total[b] != honest_total[b]).any()]
    print(f"forged cpu column {names[col]} row {row}: oracle names bus {bad_bus}, GPU unbalanced buses {nonzero}")
    assert bad_bus in nonzero
    p.job_free(job)
    p.pk_free(pk)
    p.close()
