"""Phase 1 on several prover lanes ("phase1_lanes": 1..lanes) gives the headers and the bytes of the one-lane prover: a
shard's header depends only on the shard and the key, whichever lane (stream, arena, pool) committed it, and the job keeps
its shards in execution order.  Each case compares against "lanes": 1, whose proof must verify."""
import numpy as np
import pytest

from tests import guests
from tests.test_gpu_multi_device import _late
from tests.test_gpu_phase2_lanes import _per_shard, _precompile_guest

pytestmark = pytest.mark.gpu

Q, POW = 8, 4


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    yield


def _prover(log_shard, extra):
    from dvt_circuits_amd import capi

    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


def _lanes(lanes, phase1):
    return ', "lanes": %d, "phase1_lanes": %d' % (lanes, phase1)


def _three_ways(p, elf, stdin):
    """(headers, container of the per-shard loop, prove_job container, prove_core container, vk)"""
    pk, vk = p.setup(elf)
    job, headers, _, proofs = _per_shard(p, pk, vk, stdin)
    loop = p.assemble(job, proofs)
    p.job_free(job)
    job, _ = p.prepare(pk, stdin)
    whole = p.prove_job(pk, job)
    p.job_free(job)
    core, _ = p.prove_core(pk, stdin)
    p.pk_free(pk)
    return [headers[i] for i in range(len(proofs))], loop, whole, core, vk


def _same_headers(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def reference(gpu):
    """the 13-shard job on one lane, keep_phase1 1: (elf, headers, container, vk); the container verifies"""
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(1, limbs=12)
    p = _prover(10, ', "lanes": 1')
    headers, loop, whole, core, vk = _three_ways(p, elf, ())
    p.close()
    assert len(headers) == 13 and loop == whole == core
    ok, ec, pv, why = capi.verify(vk, loop, Q, POW)
    assert ok and ec == 0 and pv == want, why
    return elf, headers, loop, vk


@pytest.mark.parametrize("keep", [1, 0])
def test_phase1_lanes_reproduce_the_one_lane_bytes(reference, keep):
    """1, 2 and 3 committing lanes of 3: the 13 headers and the container by the per-shard loop, prove_job and prove_core"""
    elf, ref_headers, ref, ref_vk = reference
    if keep == 0:   # (the one-lane recompute path gives the same bytes as the kept one)
        p = _prover(10, ', "lanes": 1, "keep_phase1": 0')
        headers, loop, whole, core, vk = _three_ways(p, elf, ())
        p.close()
        assert _same_headers(headers, ref_headers) and loop == whole == core == ref and vk == ref_vk
    for phase1 in (1, 2, 3):
        p = _prover(10, _lanes(3, phase1) + ', "keep_phase1": %d' % keep)
        headers, loop, whole, core, vk = _three_ways(p, elf, ())
        p.close()
        assert vk == ref_vk
        assert _same_headers(headers, ref_headers), "phase1_lanes %d: headers differ from the one-lane job's" % phase1
        for way, got in enumerate((loop, whole, core)):
            assert got == ref, "phase1_lanes %d, way %d: bytes differ from the one-lane proof" % (phase1, way)


def test_shard_order_does_not_depend_on_the_committing_lane(reference):
    """three two-lane prepares in one process: the same shard count and the same header at every position"""
    elf, ref_headers, _, _ = reference
    p = _prover(10, _lanes(2, 2))
    pk, _ = p.setup(elf)
    for _ in range(3):
        job, _ = p.prepare(pk, ())
        assert p.job_shards(job) == len(ref_headers)
        headers = [p.commit_shard(pk, job, i) for i in range(len(ref_headers))]
        p.job_free(job)
        assert _same_headers(headers, ref_headers)
    p.pk_free(pk)
    p.close()


def test_phase1_lanes_on_a_partial_job(reference):
    """prepare_part(first=1, stride=2), the multi-rank shape, committed on two lanes: headers and shard proofs of the held
    shards equal the full one-lane job's"""
    elf, ref_headers, _, _ = reference
    p1 = _prover(10, ', "lanes": 1')
    pk1, vk = p1.setup(elf)
    job, _, ch, ref = _per_shard(p1, pk1, vk, ())
    n = p1.job_shards(job)
    p1.job_free(job)
    p1.pk_free(pk1)
    p1.close()
    p2 = _prover(10, _lanes(2, 2))
    pk2, vk2 = p2.setup(elf)
    assert vk2 == vk
    job, part_headers, _, got = _per_shard(p2, pk2, vk2, (), first=1, stride=2, ch=ch)
    assert sorted(part_headers) == list(range(1, n, 2))
    for i in part_headers:
        assert np.array_equal(part_headers[i], ref_headers[i])
    assert got == [ref[i] for i in range(1, n, 2)]
    p2.job_free(job)
    p2.pk_free(pk2)
    p2.close()


def test_phase1_lanes_with_sha_and_curve_precompile_chips(gpu):
    """the wide short tables and the device-built auxiliary rows of the precompile chips go through the feeder's upload"""
    from dvt_circuits_amd import capi

    elf, stdin, want = _precompile_guest()
    p = _prover(12, ', "lanes": 1')
    ref = _three_ways(p, elf, stdin)
    p.close()
    assert ref[1] == ref[2] == ref[3]
    ok, ec, pv, why = capi.verify(ref[4], ref[1], Q, POW)
    assert ok and ec == 0 and pv == want, why
    p = _prover(12, _lanes(2, 2))
    got = _three_ways(p, elf, stdin)
    p.close()
    assert _same_headers(got[0], ref[0])
    assert got[1:] == ref[1:]


def test_two_members_on_one_device_with_two_phase1_lanes_each(reference):
    """"devices": [0, 0] and two phase-1 lanes per member: four committers take turns at the admission of their shards"""
    elf, ref_headers, ref, ref_vk = reference
    p = _prover(10, _lanes(2, 2) + ', "devices": [0, 0]')
    headers, loop, whole, core, vk = _three_ways(p, elf, ())
    p.close()
    assert vk == ref_vk and _same_headers(headers, ref_headers)
    assert loop == ref and whole == ref and core == ref


def test_reuse_after_a_guest_trap(reference):
    """a guest that traps in its sixth shard (reported by the executor): the code and the text of one lane, and the next job
    on the same handle gives the reference bytes"""
    from dvt_circuits_amd import capi

    elf, _, ref, _ = reference
    bad = _late("trap", loops=2800)
    rc, rep, _, _ = capi.execute(bad)
    assert rc == capi.DVT_ERR_GUEST and 5 * 1024 < rep["cycles"] <= 6 * 1024
    seen = []
    for extra in (', "lanes": 1', _lanes(2, 2)):
        p = _prover(10, extra)
        for call in ("prove_core", "prepare"):
            pk, _ = p.setup(bad)
            with pytest.raises(capi.DvtError) as e:
                getattr(p, call)(pk, ())
            seen.append((call, e.value.code, e.value.msg))
            p.pk_free(pk)
            pk, _ = p.setup(elf)
            assert p.prove_core(pk, ())[0] == ref
            p.pk_free(pk)
        p.close()
    assert seen[:2] == seen[2:]
    assert all(code == capi.DVT_ERR_GUEST for _, code, _ in seen)


def test_single_shard_job(gpu):
    """a job of one shard has nothing for a second lane (none is made for it); its bytes are the one-lane bytes"""
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(1, limbs=12)
    out = []
    for extra in (', "lanes": 1', _lanes(2, 2)):
        p = _prover(14, extra)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, ())
        assert p.job_shards(job) == 1
        p.job_free(job)
        out.append((p.prove_core(pk, ())[0], vk))
        p.pk_free(pk)
        p.close()
    assert out[0] == out[1]
    ok, ec, pv, why = capi.verify(out[0][1], out[0][0], Q, POW)
    assert ok and ec == 0 and pv == want, why


@pytest.mark.parametrize("lanes,phase1", [(2, 0), (2, 3), (1, 2), (3, 4)])
def test_phase1_lane_count_out_of_range_is_refused(gpu, lanes, phase1):
    from dvt_circuits_amd import capi

    with pytest.raises(capi.DvtError) as e:
        _prover(10, _lanes(lanes, phase1))
    assert e.value.code == capi.DVT_ERR_INPUT and "phase1_lanes" in e.value.msg
