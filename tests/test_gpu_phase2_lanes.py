"""Phase 2 on several prover lanes ("lanes": 1..3) gives the bytes of the one-lane prover: every shard proof depends only on
the shard, the key and the common challenges, whichever lane (stream, arena, pool) proves it.  Each case compares against
"lanes": 1 and checks that the proof verifies."""
import numpy as np
import pytest

from tests import guests

pytestmark = pytest.mark.gpu

Q, POW = 8, 4


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    yield


def _prover(lanes, log_shard, extra=""):
    from dvt_circuits_amd import capi

    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d, "lanes": %d%s}' % (Q, POW, log_shard, lanes, extra))


def _per_shard(p, pk, vk, stdin, first=0, stride=1, ch=None):
    """the bench's loop: prepare -> commit_shard -> challenges -> prove_shard for each held shard"""
    from dvt_circuits_amd import capi

    job, _ = p.prepare(pk, stdin, first=first, stride=stride)
    n = p.job_shards(job)
    mine = list(range(first, n, stride))
    headers = {i: p.commit_shard(pk, job, i) for i in mine}
    if ch is None:
        assert stride == 1
        ch = capi.rv32_challenges(vk, [headers[i] for i in range(n)])
    proofs = [p.prove_shard(pk, job, i, ch) for i in mine]
    return job, headers, ch, proofs


def _three_ways(lanes, elf, stdin, log_shard, extra=""):
    """(container of the per-shard loop, prove_job container, prove_core container, vk)"""
    p = _prover(lanes, log_shard, extra)
    pk, vk = p.setup(elf)
    job, _, _, proofs = _per_shard(p, pk, vk, stdin)
    assert len(proofs) >= 5 and len(proofs) % 2 == 1
    loop = p.assemble(job, proofs)
    p.job_free(job)
    job, _ = p.prepare(pk, stdin)
    whole = p.prove_job(pk, job)
    p.job_free(job)
    core, _ = p.prove_core(pk, stdin)
    p.pk_free(pk)
    p.close()
    return loop, whole, core, vk


@pytest.mark.parametrize("keep", [1, 0])
def test_lanes_reproduce_the_one_lane_bytes(gpu, keep):
    """an odd number of shards (13), proven by the per-shard loop, prove_job and prove_core with 1, 2 and 3 lanes"""
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(1, limbs=12)
    extra = ', "keep_phase1": %d' % keep
    ref = _three_ways(1, elf, (), 10, extra)
    assert ref[0] == ref[1] == ref[2]
    ok, ec, pv, why = capi.verify(ref[3], ref[0], Q, POW)
    assert ok and ec == 0 and pv == want, why
    for lanes in (2, 3):
        got = _three_ways(lanes, elf, (), 10, extra)
        assert got[3] == ref[3]
        for k in range(3):
            assert got[k] == ref[0], "lanes %d, way %d: bytes differ from the one-lane proof" % (lanes, k)


def _precompile_guest():
    from dvt_circuits_amd import capi

    with open(guests.__file__.rsplit("/", 1)[0] + "/golden/finalization_example.json", "rb") as f:
        buf = capi.stdin_from_json("finalization", f.read())
    elf = guests.dkg_like("finalization", 1, 1, 1, sha_precompiles=True, curve_precompiles=True)
    want = guests.dkg_like_expected(buf, "finalization", 1, 1, 1, curve_precompiles=True)
    return elf, [buf], want


def test_lanes_with_sha_and_curve_precompile_chips(gpu):
    """shards with the short and wide precompile tables (part-parallel K4 / K5 launches) on two lanes"""
    from dvt_circuits_amd import capi

    elf, stdin, want = _precompile_guest()
    ref = _three_ways(1, elf, stdin, 12)
    got = _three_ways(2, elf, stdin, 12)
    assert ref[0] == ref[1] == ref[2]
    assert got[:3] == ref[:3]
    ok, ec, pv, why = capi.verify(ref[3], ref[0], Q, POW)
    assert ok and ec == 0 and pv == want, why


def test_lanes_on_a_partial_job(gpu):
    """prepare_part(first=1, stride=2), the multi-rank shape: the held shards' proofs equal the one-lane full job's"""
    elf, want = guests.bignum(1, limbs=12)
    p1 = _prover(1, 10)
    pk1, vk = p1.setup(elf)
    job, headers, ch, ref = _per_shard(p1, pk1, vk, ())
    n = p1.job_shards(job)
    p1.job_free(job)
    p2 = _prover(2, 10)
    pk2, vk2 = p2.setup(elf)
    assert vk2 == vk
    job, part_headers, _, got = _per_shard(p2, pk2, vk2, (), first=1, stride=2, ch=ch)
    for i in part_headers:
        assert np.array_equal(part_headers[i], headers[i])
    assert got == [ref[i] for i in range(1, n, 2)]
    p2.job_free(job)
    for p, pk in ((p1, pk1), (p2, pk2)):
        p.pk_free(pk)
        p.close()


def test_early_exit_and_changed_challenges(gpu):
    """claim one shard and free the job (no hang; the next job's bytes still match), and a second prove_shard with other
    challenges gives what one lane gives for those challenges"""
    elf, _ = guests.bignum(1, limbs=12)
    p1 = _prover(1, 10)
    pk1, vk = p1.setup(elf)
    job, _, ch, ref = _per_shard(p1, pk1, vk, ())
    p1.job_free(job)
    other = np.array(ch, dtype=np.uint32).copy()
    other[0] = (int(other[0]) + 1) % 0x78000001
    job, _ = p1.prepare(pk1, ())
    ref_other = p1.prove_shard(pk1, job, 3, other)
    p1.job_free(job)

    p2 = _prover(2, 10)
    pk2, _ = p2.setup(elf)
    job, _ = p2.prepare(pk2, ())
    assert p2.prove_shard(pk2, job, 0, ch) == ref[0]
    p2.job_free(job)
    job, _, _, got = _per_shard(p2, pk2, vk, ())
    assert got == ref
    p2.job_free(job)
    job, _ = p2.prepare(pk2, ())
    assert p2.prove_shard(pk2, job, 2, ch) == ref[2]
    assert p2.prove_shard(pk2, job, 3, other) == ref_other
    assert p2.prove_shard(pk2, job, 4, ch) == ref[4]
    p2.job_free(job)
    for p, pk in ((p1, pk1), (p2, pk2)):
        p.pk_free(pk)
        p.close()


@pytest.mark.parametrize("lanes", [0, 4])
def test_lane_count_out_of_range_is_refused(gpu, lanes):
    from dvt_circuits_amd import capi

    with pytest.raises(capi.DvtError) as e:
        _prover(lanes, 10)
    assert e.value.code == capi.DVT_ERR_INPUT
