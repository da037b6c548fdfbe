"""GPU tests of Prover.verify / Prover.machine_verify (the query part of the verifier on the device) against the host
verifier: the same decision and the same text on the committed fixtures, on hundreds of tampered copies (most of which
reach the hashing kernels), on a multi-shard proof made here, on toy-machine proofs with the smallest trees, and a prove -
check - verify - prove sequence that leaves the handle's job state alone."""
import os
import struct

import numpy as np
import pytest

from tests import guests, toy_traces

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, POW = 4, 4
P = 2013265921
TREE, LAYER = "Merkle opening rejected (input tree)", "Merkle opening rejected (FRI layer)"


def _load(name):
    from dvt_circuits_amd import capi

    blob = open(os.path.join(ROOT, "tests", "golden", f"proof_{name}.bin"), "rb").read()
    (n,) = struct.unpack_from("<I", blob)
    vk, proof = blob[4:4 + n], blob[4 + n:]
    assert capi.verify(vk, proof, Q, POW)[0], "stale fixture"
    return vk, proof


@pytest.fixture(scope="module")
def prover():
    from dvt_circuits_amd import capi

    p = capi.Prover('{"fri_queries": 6, "pow_bits": 5, "log_shard_size": 10}')
    yield p
    p.close()


def _tamper(words, pos):
    w = words.copy()
    w[pos] = (int(w[pos]) + 1) % P if w[pos] < P else int(w[pos]) - 1
    return w.tobytes()


def test_fixtures_are_accepted_and_rejected_like_the_host(prover):
    from dvt_circuits_amd import capi

    vk, proof = _load("commit")
    vk2, proof2 = _load("curve")
    for args in ((vk, proof, Q, POW), (vk2, proof2, Q, POW), (vk2, proof, Q, POW), (vk, proof2, Q, POW), (vk, proof, Q + 1, POW),
                 (vk, proof, Q, POW + 1)):
        assert prover.verify(*args) == capi.verify(*args)
    ok, ec, pv, _ = prover.verify(vk, proof, Q, POW)
    assert ok and ec == 0 and pv == b"fuzz me!"
    assert prover.verify(vk2, proof2, Q, POW)[0]
    print("fixture verify on the device:", prover.verify_times())


@pytest.mark.parametrize("name", ["commit", "curve"])
def test_tampered_words_get_the_hosts_reason(prover, name):
    from dvt_circuits_amd import capi

    vk, proof = _load(name)
    words = np.frombuffer(proof, np.uint32).copy()
    # the positions of test_every_tampered_word_is_rejected (same seed, same rule), and as many from a second seed
    pos = list(range(0, 12)) + [int(x) for x in np.random.default_rng(9).integers(12, len(words), 120)]
    pos += [int(x) for x in np.random.default_rng(11).integers(12, len(words), 120)]
    host_reasons = []
    for at in pos:
        bad = _tamper(words, at)
        host = capi.verify(vk, bad, Q, POW)
        assert not host[0]
        host_reasons.append(host[3])
        assert prover.verify(vk, bad, Q, POW) == host, f"{name}: word {at}"
    # the inputs reach the kernels: most failures are hash failures of both kinds
    tree = sum(TREE in r for r in host_reasons)
    layer = sum(LAYER in r for r in host_reasons)
    assert tree and layer and 2 * (tree + layer) > len(pos), (tree, layer, len(pos))
    for bad in (proof[:-4], proof + b"\0\0\0\0", proof[:len(proof) // 2], proof[:-3]):
        assert prover.verify(vk, bad, Q, POW) == capi.verify(vk, bad, Q, POW)


def _shard_spans(words):
    """(position of the length word, first word, one past the last word) of every shard payload of a container"""
    n, pvl = int(words[1]), int(words[3])
    at = 4 + (pvl + 3) // 4
    out = []
    for _ in range(n):
        out.append((at, at + 1, at + 1 + int(words[at])))
        at = out[-1][2]
    assert at == len(words)
    return out


@pytest.fixture(scope="module")
def three_shards(prover):
    elf = guests.commit_only(b"check me")
    pk, vk = prover.setup(elf)
    proof, rep = prover.prove_core(pk, [])
    prover.pk_free(pk)
    words = np.frombuffer(proof, np.uint32).copy()
    assert len(_shard_spans(words)) >= 3
    return vk, proof, words


def test_multi_shard_proof_and_the_order_of_failures(prover, three_shards):
    from dvt_circuits_amd import capi

    q, pw = 6, 5
    vk, proof, words = three_shards
    spans = _shard_spans(words)
    ok, ec, pv, why = prover.verify(vk, proof, q, pw)
    assert ok and pv == b"check me" and (ok, ec, pv, why) == capi.verify(vk, proof, q, pw), why
    t = prover.verify_times()
    print("three-shard verify on the device:", t)
    assert t["permutations"] > 0 and t["launches"] == 4 * t["chunks"]
    # one word in the query section of shard 2 and one in shard 3 (the last words of a payload are a FRI path)
    w = words.copy()
    for s in (1, 2):
        at = spans[s][2] - 5
        w[at] = (int(w[at]) + 1) % P
    host = capi.verify(vk, w.tobytes(), q, pw)
    assert not host[0] and host[3].startswith("shard 2: Merkle opening rejected")
    assert prover.verify(vk, w.tobytes(), q, pw) == host
    # two changes in different queries of one shard: the query section is the tail of the payload, one query is 1 / q of it
    w = words.copy()
    lo, hi = spans[1][1], spans[1][2]
    for at in (hi - 5, hi - 5 - (hi - lo) // 4):
        w[at] = (int(w[at]) + 1) % P
    host = capi.verify(vk, w.tobytes(), q, pw)
    assert not host[0] and prover.verify(vk, w.tobytes(), q, pw) == host
    # a host-part failure in shard 1 comes before a query failure in shard 1 and after nothing
    w = words.copy()
    w[spans[0][1] + 3] = (int(w[spans[0][1] + 3]) + 1) % P
    w[spans[0][2] - 5] = (int(w[spans[0][2] - 5]) + 1) % P
    host = capi.verify(vk, w.tobytes(), q, pw)
    assert not host[0] and prover.verify(vk, w.tobytes(), q, pw) == host
    # the last word of one payload dropped, the length word fixed up
    for s in (0, 2):
        w = np.concatenate([words[:spans[s][2] - 1], words[spans[s][2]:]])
        w[spans[s][0]] -= 1
        host = capi.verify(vk, w.tobytes(), q, pw)
        assert not host[0] and prover.verify(vk, w.tobytes(), q, pw) == host, host[3]
    # a spread of single-word changes over all shards
    rng = np.random.default_rng(3)
    for at in rng.integers(spans[0][0], len(words), 60):
        bad = _tamper(words, int(at))
        assert prover.verify(vk, bad, q, pw) == capi.verify(vk, bad, q, pw), int(at)


@pytest.mark.parametrize("log_n", [1, 2, 3, 6])
def test_toy_machine_proofs(prover, log_n):
    from dvt_circuits_amd import capi

    q, pw = 6, 5
    prep, main, pubs = toy_traces.build(log_n, max(log_n - 2, 0), 1)
    pk, vk = prover.machine_setup("toy", prep)
    proof = prover.machine_prove(pk, main, pubs)
    prover.pk_free(pk)
    assert capi.machine_verify(vk, proof, q, pw) == (True, "")
    assert prover.machine_verify(vk, proof, q, pw) == (True, "")
    assert prover.machine_verify(vk, proof, q + 1, pw) == capi.machine_verify(vk, proof, q + 1, pw)
    words = np.frombuffer(proof, np.uint32).copy()
    rng = np.random.default_rng(20 + log_n)
    hashes = 0
    for at in rng.integers(0, len(words), 40):
        bad = _tamper(words, int(at))
        host = capi.machine_verify(vk, bad, q, pw)
        assert not host[0]
        hashes += "Merkle opening" in host[1]
        assert prover.machine_verify(vk, bad, q, pw) == host, int(at)
    assert hashes, "no tampered word reached a Merkle opening"


def test_verify_leaves_the_job_state_alone(prover):
    elf = guests.commit_only(b"check me")
    pk, vk = prover.setup(elf)
    job, _ = prover.prepare(pk, [])
    first = prover.prove_job(pk, job)
    prover.check_job(pk, job)
    assert prover.verify(vk, first, 6, 5)[0]
    assert prover.prove_job(pk, job) == first
    assert prover.verify(vk, first, 6, 5)[0]
    prover.job_free(job)
    prover.pk_free(pk)
