"""GPU test of K0 of the five big-integer precompile chips (csrc/rv32_bigops.hip: k0_bigop_cells / _rels / _lookups
kernels) on the extremes corpus of tests/_bigop_corpus.py.  The device solves the identities' witnesses with another
algorithm than the host (one wave per row, solve_poly_rel_wave; for u256_mul a long division on lane 0), so its rows are
compared, exactly and cell by cell, with (a) the Python model's rows (oracle/rv32_model.py: plain integers) and (b) the
product's host rows (polyrel.h solve_poly_rel).  All chips of a shard are compared: the lookups kernel's counts land in
the byte chip.  65..130 rows per chip and 264 for u256_mul: just past the 64- and 256-thread workgroups of the cells and
lookups kernels; at log_shard_size = 8 the calls spread over several shards, so the shard number and the cross-shard
timestamps of the operands vary."""
import numpy as np
import pytest

from tests import _bigop_corpus as corpus

pytestmark = pytest.mark.gpu


def _same(kind, shard, want, got):
    assert len(want) == len(got), (kind, shard, [c["chip_id"] for c in want], [c["chip_id"] for c in got])
    for w, g in zip(want, got):
        assert w["chip_id"] == g["chip_id"] and w["log_n"] == g["log_n"], (kind, shard, w["chip_id"], g["chip_id"], w["log_n"], g["log_n"])
        diff = np.argwhere(w["main"] != g["main"])
        detail = [(int(c), int(r), int(w["main"][c, r]), int(g["main"][c, r])) for c, r in diff[:12]]
        assert diff.size == 0, f"shard {shard} chip {w['chip_id']}: {len(diff)} cells differ from the {kind}, first (col,row,{kind},dev): {detail}"


@pytest.mark.parametrize("log_shard", [21, 8])
@pytest.mark.parametrize("chip", corpus.CHIPS)
def test_k0_device_rows_equal_model_and_host_rows_on_the_extremes(chip, log_shard):
    from dvt_circuits_amd import capi

    elf, _ = corpus.guest(chip)
    cid = corpus.air_chip(chip)[0]
    run = corpus.model_run(chip, log_shard)
    p = capi.Prover('{"fri_queries": 8, "pow_bits": 4, "log_shard_size": %d}' % log_shard)
    pk, vk = p.setup(elf)
    job, rep = p.prepare(pk, [])
    n = p.job_shards(job)
    assert n == len(run.shards) and rep["cycles"] == run.cycles and (n == 1 if log_shard == 21 else n >= 4)
    rows, shards_with_rows = 0, 0
    for shard in range(n):
        host, hpubs, hn = capi.rv32_debug_traces(elf, (), log_shard, shard)
        dev, dpubs = p.debug_device_traces(pk, job, shard)
        model, mpubs = corpus.model_traces(chip, log_shard, shard)
        assert hn == n and (dpubs == mpubs).all() and (dpubs == hpubs).all()
        _same("model", shard, model, dev)
        _same("host", shard, host, dev)
        own = corpus.chip_rows(chip, dev)
        if own is not None:
            rows += own.shape[1]
            shards_with_rows += 1
    assert rows == len(corpus.cases(chip)) and (shards_with_rows >= 2 if log_shard == 8 else shards_with_rows == 1)
    if log_shard == 21:
        # the GPU's own constraint evaluation and bus balance accept the extreme rows, and the proof over them verifies
        summary, findings = p.check_job(pk, job)
        assert summary["ok"] and summary["violations"] == 0 and findings == [] and summary["unbalanced_buses"] == 0, (summary, findings)
        assert p.job_shard_chips(job, 0) >> cid & 1
        proof = p.prove_job(pk, job)
        ok, ec, pv, why = capi.verify(vk, proof, 8, 4)
        assert ok and ec == 0 and pv == run.public_values, why
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_quotient_overflow_traps_in_the_executor():
    """UINT256_MUL with floor(x * y / m) >= 2^264 has no row (the chip's quotient has 33 bytes): the executor traps, the
    prover reports the guest's error and asks the device for no row"""
    from dvt_circuits_amd import capi
    from tests.guests_bigops import precompile_calls
    from tests.guests import SYS_UINT256_MUL, words_of

    elf, _ = precompile_calls([(SYS_UINT256_MUL, words_of(1 << 132, 8), words_of(1 << 132, 8) + words_of(1, 8))])
    p = capi.Prover('{"fri_queries": 8, "pow_bits": 4}')
    pk, _ = p.setup(elf)
    with pytest.raises(capi.DvtError) as ei:
        p.prepare(pk, [])
    assert ei.value.code == capi.DVT_ERR_GUEST and "UINT256_MUL" in str(ei.value) and "2^264" in str(ei.value), str(ei.value)
    p.pk_free(pk)
    p.close()
