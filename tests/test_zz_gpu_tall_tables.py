"""End-to-end byte parity with precompile tables taller than 2^15 rows (collected late on purpose, like the full-size
file: it is slow).  At that height K4 runs perm_rows_kernel<Air> (all interactions of a row in one thread) and K5 one
quotient_kernel<Air, PART> launch per part, the kernels the short tables of the other guests never reach at the default
configuration.  Each guest (guests.tall_precompiles) is proven at the default configuration; the proof must verify and
its shard must equal the oracle CPU prover's, byte for byte.  As in test_zz_gpu_fullsize_parity.py the oracle is fed the
product's host row expansion (capi.rv32_debug_traces): the Python model is too slow at this size; the rows themselves
are checked by tests/test_tall_precompile_guests.py (constraints) and tests/test_gpu_k0_parity.py (K0)."""
import pytest

from dvt_circuits_amd.capi import split_container
from tests import _oracle_prover, guests
from tests.test_gpu_proof_parity import first_diff

pytestmark = pytest.mark.gpu
Q, POW, LOG_SHARD = 6, 5, 17
CHIP_ID = {"fp_op": 9, "fp2_op": 10, "bls_g1": 11, "secp_k1": 12, "u256_mul": 13}


@pytest.mark.parametrize("chip", guests.TALL_CHIPS)
def test_tall_precompile_table_proof_equals_oracle(chip):
    from dvt_circuits_amd import capi

    elf, want = guests.tall_precompiles(chip)
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d}' % (Q, POW, LOG_SHARD))
    pk, vk = p.setup(elf)
    proof, rep = p.prove_core(pk, [])
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and ec == 0 and pv == guests.checksum(want), why
    ec, _, gpu = split_container(proof)
    assert len(gpu) == 1
    chips, pubs, n = capi.rv32_debug_traces(elf, [], LOG_SHARD, 0)
    assert n == 1 and any(c["chip_id"] == CHIP_ID[chip] and c["log_n"] >= 16 for c in chips)
    gc = _oracle_prover.global_challenges(_oracle_prover.prep_root_of(chips), [_oracle_prover.main_root(chips) + [int(x) for x in pubs]])
    cpu, _ = _oracle_prover.prove_shard("rv32", chips, pubs, Q, POW, perm_challenges=gc)
    assert gpu[0] == cpu, f"first differing word / lengths: {first_diff(gpu[0], cpu)}"
    p.pk_free(pk)
    p.close()
