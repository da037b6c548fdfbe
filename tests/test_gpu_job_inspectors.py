"""GPU test of the four job-level inspectors (check_job, job_bus_tuples, hunt_shard, hunt_join_job) run one after the other
on one prepared job, before and after it is proven, with and without the phase-1 results kept in HBM.  With "keep_phase1": 0
a shard has no buffers of its own: every inspector runs K0 into the lane's working buffers, which the next shard's K0
overwrites, and the shard's traces never count as valid.  Either way the answers are the same and the job stays as found:
both proofs of the inspected job are the bytes of a job that was never inspected."""
import functools

import pytest

from tests import guests

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
P = 2013265921
CPU = 2
DELTAS = [1, P - 1]
HUNT = dict(shard=1, row=5)   # the shard no join window is on
JOIN_ROWS = 4                 # cpu rows per window, on the first and on the last shard


def _inspect(p, pk, job):
    summary, findings = p.check_job(pk, job)
    assert summary["ok"] and summary["violations"] == 0 and findings == [], summary
    assert summary["bus_checked"] == 1 and summary["unbalanced_buses"] == 0, summary
    assert p.job_bus_tuples(pk, job) == ([], False)
    counts, fmap = p.hunt_shard(pk, job, HUNT["shard"], CPU, DELTAS, row_first=HUNT["row"], row_count=1)
    join = p.hunt_join_job(pk, job, [(0, CPU, 0, JOIN_ROWS), (2, CPU, 0, JOIN_ROWS)], DELTAS)
    main_w = p.job_shard_chip_shape(job, 0, CPU)[0]
    assert join["summary"]["candidates"] == 2 * JOIN_ROWS * main_w * len(DELTAS) and join["summary"]["truncated"] == 0
    return counts.tolist(), fmap.tolist(), join


@functools.lru_cache(maxsize=None)
def _answers(keep):
    """the hunt and join answers of a three-shard job before its proof; asserts everything else"""
    from dvt_circuits_amd import capi

    cfg = '{"fri_queries": %d, "pow_bits": %d, "log_shard_size": 11, "keep_phase1": %d}' % (Q, POW, keep)
    elf, want = guests.commit_only(b"check me"), b"check me"
    proofs, answers = [], []
    for inspect in (True, False):
        p = capi.Prover(cfg)
        try:
            pk, vk = p.setup(elf)
            job, _ = p.prepare(pk, [])
            assert p.job_shards(job) == 3
            for _ in range(2 if inspect else 1):   # (the second proof starts from consumed phase-1 results)
                if inspect:
                    answers.append(_inspect(p, pk, job))
                proofs.append(p.prove_job(pk, job))
            p.job_free(job)
            p.pk_free(pk)
        finally:
            p.close()
    assert answers[0] == answers[1]
    assert proofs[0] == proofs[2] and proofs[1] == proofs[2]
    ok, ec, pv, why = capi.verify(vk, proofs[2], Q, POW)
    assert ok and ec == 0 and pv == want, why
    return answers[0]


@pytest.mark.parametrize("keep", (1, 0))
def test_inspectors_leave_the_job_as_found(keep):
    assert _answers(keep) == _answers(1)
