"""Byte parity of the row-parallel K4 / K5 launches on small tables.  Tables of at most 2^parts_parallel_log rows (default
2^15) take the part-parallel launches (perm_rows_parts_kernel / quotient_parts_kernel + sum_parts_kernel), taller ones
perm_rows_kernel and one quotient_kernel<Air, PART> launch per part (dvt_circuits_amd/csrc/machine.h).  Every precompile
table of the test guests is short, so at the default those row-parallel kernels of the precompile chips never run.
{"parts_parallel_log": -1} forces them at every height: the proof must equal the oracle's bytes and the default-config
proof's bytes (the launch split does not enter the transcript).

Coverage: with the switch at -1 every chip of a shard runs perm_rows_kernel<Air> (if it has interactions) and
quotient_kernel<Air, PART> for all of its parts, so the instantiations run are exactly those of the chips present in the
shards.  test_forced_cases_cover_every_chip (no GPU) reads the chip list of every shard of every case below from
capi.rv32_debug_traces and requires all rv32 chips; the toy case covers the toy machine's three chips."""
import numpy as np
import pytest

from dvt_circuits_amd.capi import split_container
from tests import guests, toy_traces
from tests.test_gpu_proof_parity import Q, POW, first_diff, oracle_prove_execution

FORCED = '"parts_parallel_log": -1'
# guest, log_shard: the small shapes of test_gpu_proof_parity.py, one per chip family
CASES = [("field_ops", 9), ("curve_ops", 8), ("u256_ops", 7), ("sha_extend", 9), ("sha256_precompiled", 10), ("bignum", 8),
         ("muldiv", 10), ("shifts", 9)]


def _guest(which):
    if which == "bignum":
        elf, want = guests.bignum(2, limbs=3)
        return elf, want
    elf, want = getattr(guests, which)()
    return elf, guests.checksum(want)


def test_forced_cases_cover_every_chip():
    """the chips present in the shards of CASES: all of the rv32 machine's (so every perm_rows_kernel and every
    quotient_kernel<Air, PART> instantiation of it runs under the forced switch)"""
    from dvt_circuits_amd import capi
    from tests import _orc

    air = _orc.air("rv32")
    seen, wide = set(), set()
    for which, log_shard in CASES:
        elf, _ = _guest(which)
        shard, n = 0, 1
        while shard < n:
            chips, _, n = capi.rv32_debug_traces(elf, [], log_shard, shard)
            for c in chips:
                seen.add(c["chip_id"])
                if c["chip_id"] >= 7:
                    wide.add((air.chip(c["chip_id"]).name.decode(), int(c["log_n"])))
            shard += 1
    assert seen == set(range(air.nchips)), f"chips never present: {sorted(set(range(air.nchips)) - seen)}"
    # and at the default they would all have taken the part-parallel launches
    assert all(log_n <= 15 for _, log_n in wide), wide


@pytest.mark.gpu
@pytest.mark.parametrize("which,log_shard", CASES)
def test_row_parallel_proof_equals_oracle_and_default(which, log_shard):
    from dvt_circuits_amd import capi

    elf, want = _guest(which)
    shards = {}
    for mode in ("default", "forced"):
        p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, ", " + FORCED if mode == "forced" else ""))
        pk, vk = p.setup(elf)
        proof, _ = p.prove_core(pk, [])
        ec, pv, shards[mode] = split_container(proof)
        assert ec == 0 and pv == want
        assert capi.verify(vk, proof, Q, POW)[0]
        p.pk_free(pk)
        p.close()
    cpu = oracle_prove_execution(elf, (), log_shard)
    assert len(shards["forced"]) == len(shards["default"]) == len(cpu) > 1
    for i, (f, d, c) in enumerate(zip(shards["forced"], shards["default"], cpu)):
        assert f == c, f"forced row-parallel path, shard {i}: first differing word / lengths: {first_diff(f, c)}"
        assert d == c, f"default path, shard {i}: first differing word / lengths: {first_diff(d, c)}"


@pytest.mark.gpu
def test_row_parallel_toy_proof_equals_oracle_and_default():
    from dvt_circuits_amd import capi
    from tests import _oracle_prover

    prep, main, pubs = toy_traces.build(9, 11, 1500)
    proofs = []
    for cfg in ("", ", " + FORCED):
        p = capi.Prover('{"fri_queries": %d, "pow_bits": %d%s}' % (Q, POW, cfg))
        pk, vk = p.machine_setup("toy", prep)
        proofs.append(p.machine_prove(pk, main, pubs))
        p.pk_free(pk)
        p.close()
    chips = [dict(chip_id=cid, main=m, prep=(prep[0][1] if cid == toy_traces.RANGE8 else np.zeros((0, m.shape[1]), np.uint32))) for cid, m in main]
    cpu, _ = _oracle_prover.prove_shard("toy", chips, pubs, Q, POW)
    assert proofs[1] == cpu, f"first differing word / lengths: {first_diff(proofs[1], cpu)}"
    assert proofs[0] == cpu


@pytest.mark.gpu
@pytest.mark.parametrize("value", [16, 22, -2])
def test_parts_parallel_log_out_of_range_is_refused(value):
    """above 15 the d_parts scratch of the engine (sized for 2^15 rows) would overflow"""
    from dvt_circuits_amd import capi

    with pytest.raises(capi.DvtError) as e:
        capi.Prover('{"parts_parallel_log": %d}' % value)
    assert e.value.code == capi.DVT_ERR_INPUT
