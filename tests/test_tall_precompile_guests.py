"""CPU tests (no GPU) of the tall precompile guests (guests.tall_precompiles): more than 2^15 calls of one precompile in a
single shard, so that the chip's table is at least 2^16 rows tall and K4 / K5 of the prover take the row-parallel launches
(perm_rows_kernel, quotient_kernel<Air, PART>) instead of the part-parallel ones.  Here: the executor's result against
plain Python big-integer arithmetic, the height the guest was written for, and every constraint of every chip.  The GPU
side of the same guests is tests/test_zz_gpu_tall_tables.py (proofs) and tests/test_gpu_k0_parity.py (K0 rows)."""
import pytest

from dvt_circuits_amd import capi
from tests import _orc, guests
from tests.test_rv32_exec_trace import check_traces

LOG_SHARD = 17      # the smallest shard that holds any of the tall guests (about 112 k to 120 k cycles)
CHIP_ID = {"fp_op": 9, "fp2_op": 10, "bls_g1": 11, "secp_k1": 12, "u256_mul": 13}


@pytest.fixture(scope="module")
def air():
    return _orc.air("rv32")


@pytest.mark.parametrize("chip", guests.TALL_CHIPS)
def test_tall_guest_result_height_and_air(air, chip):
    elf, want = guests.tall_precompiles(chip)
    rc, rep, pv, out, err = capi.execute_io(elf)
    assert rc == 0 and rep["halted"] and not rep["unprovable"], err
    assert out == want and pv == guests.checksum(want)
    assert rep["cycles"] <= 1 << LOG_SHARD
    chips, pubs, n = capi.rv32_debug_traces(elf, [], LOG_SHARD, 0)
    assert n == 1
    heights = {air.chip(c["chip_id"]).name.decode(): int(c["log_n"]) for c in chips}
    assert air.chip(CHIP_ID[chip]).name.decode() == chip
    assert heights.get(chip, 0) >= 16, heights           # taller than the part-parallel threshold 2^15
    check_traces(air, elf, log_shard=LOG_SHARD)
