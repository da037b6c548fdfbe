"""The device verifier at the size it is made for: one full shard of 2^21 cycles at 100 queries and 16 proof-of-work
bits (trees of depth 22, about 2 500 Merkle chains) is accepted, and one changed sibling word is rejected with the host
verifier's text.  The host verifier runs once for each of the two.  Measured on an MI355X: 1.8 s for the test body (2.5 s
with the imports), most of it the guest fit and the proof; the four kernels take 0.67 ms for the shard's 42 200 permutations."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2013265921


def test_full_size_shard_on_the_device():
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    t0 = time.perf_counter()
    buf = bench.workload_stdin(0)
    elf = guests.dkg_like("finalization", *bench.fit_constants(buf, 1))
    p = capi.Prover('{"fri_queries": 100, "pow_bits": 16}')
    pk, vk = p.setup(elf)
    proof, rep = p.prove_core(pk, [buf])
    assert rep["cycles"] > 3 << 19 and len(capi.split_container(proof)[2]) == 1
    host = capi.verify(vk, proof)
    assert host[0], host[3]
    assert p.verify(vk, proof) == host
    print("full-size shard on the device:", p.verify_times())
    words = np.frombuffer(proof, np.uint32).copy()
    words[-3] = (int(words[-3]) + 1) % P        # a sibling word of the last query's last FRI path
    bad = words.tobytes()
    host = capi.verify(vk, bad)
    assert not host[0] and host[3] == "shard 1: Merkle opening rejected (FRI layer)"
    assert p.verify(vk, bad) == host
    p.pk_free(pk)
    p.close()
    print("full-size verify test: %.1f s" % (time.perf_counter() - t0))
