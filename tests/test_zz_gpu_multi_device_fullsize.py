"""Two device members on one GPU at production size: a 4-shard execution at log_shard_size 21, 100 queries, 16 proof-of-work
bits.  The one-device bytes are pinned to the oracle by tests/test_zz_gpu_fullsize_parity.py; here the [0, 0] handle must
give the same container.  This is the case in which two members of one physical device decide, shard by shard, what of
phase 1 stays in HBM (about 3 GB per shard), against the same free memory.  With 288 GB of HBM the admission says yes for
all four shards, so this case runs the kept path at size under two members; the fall-back (nothing kept, phase 2 recomputes)
under several members is covered by the keep_phase1 = 0 cases of tests/test_gpu_multi_device.py.  (Sorts late, like the
other full-size file.)"""
import pytest

from tests import guests

pytestmark = pytest.mark.gpu


def test_four_full_size_shards_on_two_members_of_one_gpu():
    import bench
    from dvt_circuits_amd import capi

    buf = bench.workload_stdin()
    consts = bench.fit_constants(buf, 4)
    elf = guests.dkg_like("finalization", *consts)
    want_pv = guests.dkg_like_expected(buf, "finalization", *consts)
    out = []
    for cfg in ('{"device": 0}', '{"devices": [0, 0]}'):
        p = capi.Prover(cfg)
        pk, vk = p.setup(elf)
        proof, rep = p.prove_core(pk, [buf])
        assert (3 << 21) < rep["cycles"] <= 4 << 21
        out.append((p.device_count(), vk, proof))
        p.pk_free(pk)
        p.close()
    assert [o[0] for o in out] == [1, 2]
    assert out[1][1] == out[0][1], "verifying key differs"
    assert len(capi.split_container(out[0][2])[2]) == 4
    assert out[1][2] == out[0][2], "the [0, 0] container differs from the one-device container"
    ok, ec, pv, why = capi.verify(out[0][1], out[1][2])
    assert ok and ec == 0 and pv == want_pv, why
