"""GPU tests of the uses slice on seeded random guests (tests/guests_random.py): Prover.job_uses on the prepared jobs of the twelve
pinned cases at 2^9 cycles per shard (thirteen or more shards of one partial workgroup each), on the positions, the pool
registers (ra in the flow cases) and the most stored scratch words of tests/test_random_guests_uses_cpu.py, the same list as the
host file's, against the rule written over the model's rows and the three yardsticks that do not depend on it.  Every
comparison is of exact integers."""
import pytest

from tests import guests_random as gr
from tests.test_random_guests_cpu import CASE_IDS, guest_of, run_of
from tests.test_random_guests_uses_cpu import LOG, check_uses

pytestmark = pytest.mark.gpu
Q, POW = 8, 4


@pytest.fixture(scope="module")
def prover():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d}' % (Q, POW, LOG))
    yield p
    p.close()


@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_job_uses_are_the_models(prover, case):
    run = run_of(case, LOG)
    pk, vk = prover.setup(guest_of(case).elf)
    job = None
    try:
        job, rep = prover.prepare(pk, [])
        assert prover.job_shards(job) == len(run.shards) >= 13 and rep["cycles"] == run.cycles
        call = lambda at, target, follow: prover.job_uses(pk, job, at, target, follow_addr=follow)
        slices, edges, uses, values = check_uses(call, case, device=True)
        print(gr.case_id(case), "slices", slices, "edges checked", edges, "uses counted", uses, "values compared", values)
        assert slices >= 2 * 3 * (10 if case[1] == "alu" else 18) and edges > 1000 and uses >= edges
    finally:
        if job is not None:
            prover.job_free(job)
        prover.pk_free(pk)
