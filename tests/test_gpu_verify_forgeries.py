"""Forged proofs against the device verifier (Prover.machine_verify / Prover.verify): the cases of tests/_forger.py, whose
transcript and Merkle trees are consistent, so that vq_reduced_kernel, vq_fold_kernel and the final-value status byte
decide.  For every case the device path, the host verifier and the forger's own prediction must agree on the decision
and on the reason.  On the rv32 machine forged shards are spliced into the five-shard container of commit_only at 2^10
cycles per shard (first failure in the host's order: shard, then query), and a handle with "verify_chunk_words" at one
shard's size runs the same container through one chunk per shard (two slots in flight, the third and the fifth chunk
reusing slot 0).

The cost is the CPU forger, not the GPU: 0.25 s per toy proof, 1.0 - 1.7 s per rv32 shard of 2^10 cycles, and 5 s once
for the rv32 model's execution and traces (measured on the host, see tests/test_verifier_forgeries.py).  The rv32
execution, its traces and its honest container are made once per module."""
import numpy as np
import pytest

from tests import _forger as F
from tests import _oracle_prover, guests, toy_traces
from tests.test_gpu_verify_parity import _shard_spans

pytestmark = pytest.mark.gpu
Q, POW = F.Q, F.POW
P = F.P


@pytest.fixture(scope="module")
def prover():
    from dvt_circuits_amd import capi

    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": 10}' % (Q, POW))
    yield p
    p.close()


# ---------------------------------------------------------------- the toy machine
@pytest.fixture(scope="module")
def toy(prover):
    """per shape: the key the library makes and the honest proof it makes"""
    out = {}
    for shape in (F.BIG, F.SMALL):
        prep, main, pubs = toy_traces.build(*shape)
        pk, vk = prover.machine_setup("toy", prep)
        out[shape] = (vk, prover.machine_prove(pk, main, pubs))
        prover.pk_free(pk)
    return out


def test_the_python_built_key_is_the_librarys(prover, toy):
    for shape, (vk, honest) in toy.items():
        chips, pubs = F.toy_chips(shape)
        assert vk == F.toy_vk(_oracle_prover.prep_root_of(chips)), shape
        assert prover.machine_verify(vk, honest, Q, POW) == (True, "")


@pytest.mark.parametrize("c", F.CASES, ids=[c["name"] for c in F.CASES])
def test_device_host_and_prediction_agree(prover, toy, c):
    from dvt_circuits_amd import capi

    vk, honest = toy[c["shape"]]
    proof, prep_root, f = F.forge_case(c)
    assert F.toy_vk(prep_root) == vk
    assert F.PATTERNS[c["pattern"]](f), f"stale constant: {c['name']}: {f.outcomes()}"
    want = f.predict()
    host = capi.machine_verify(vk, proof, c["q"], POW)
    dev = prover.machine_verify(vk, proof, c["q"], POW)
    assert dev == host, (dev, host, want)
    assert host[0] == want[0] and (host[1].startswith(want[1]) if want[1].startswith(F.ZETA) else host[1] == want[1]), (host, want)
    # the pinned staging and the status bytes of the forged proof are reused: the honest proof is still accepted
    assert prover.machine_verify(vk, honest, Q, POW) == (True, "")


# ---------------------------------------------------------------- rv32, five shards
class Rv32:
    """one execution of commit_only at 2^10 cycles per shard: the oracle's traces of every shard and the common
    challenges, from which single shards are re-proved with a cheat (cheats that leave the main root alone: the headers
    and the challenges stand)"""

    def __init__(self, elf, log_shard=10):
        from oracle import rv32_model

        run = rv32_model.Run(elf, (), log_shard)
        assert run.halted and not run.error
        self.shards = [rv32_model.traces(run, i) for i in range(len(run.shards))]
        prep_root = _oracle_prover.prep_root_of(self.shards[0][0])
        headers = [_oracle_prover.main_root(chips) + [int(x) for x in pubs] for chips, pubs in self.shards]
        self.gc = _oracle_prover.global_challenges(prep_root, headers)

    def tallest(self, i):
        return max(self.shards[i][0], key=lambda c: c["main"].shape[1])["chip_id"]

    def forge(self, i, cheats, final=0):
        chips, pubs = self.shards[i]
        f = F.Forgery(*cheats, final=final)
        return _oracle_prover.prove_shard("rv32", chips, pubs, Q, POW, perm_challenges=self.gc, cheat=f)[0], f


# The cheats of the forged shards, as functions of the tallest chip's id and of delta.  RV_DELTAS holds, like
# _forger.DELTAS, the first delta in 1..F.SEARCH_TRIES whose proof shows the pattern in RV_CASES; the tests assert the
# patterns, and `python -m tests.test_gpu_verify_forgeries` (no GPU needed) repeats the search and prints the table.
RV_DELTAS = {"last": 1, "layer": 3, "first": 1}


def RV_LAST(chip, d=None):      # the last shard: an altered quotient word of odd position; final_poly = last[0]
    return [F.lde_point("quot", chip, 5, 33, d or RV_DELTAS["last"])]


def RV_LAYER(chip, d=None):     # shard 2 (final_poly = last[1]): the layer of 4 values; a query opens value 2 before another even one fails
    return [F.layer_value(-1, 2, d or RV_DELTAS["layer"])]


def RV_FIRST(chip, d=None):     # shard 1: an altered word of the permutation tree
    return [F.lde_point("perm", chip, 1, 8, d or RV_DELTAS["first"])]


# name -> (shard position, -1 = the last; cheats; final; the pattern over the Forgery that the test asserts)
RV_CASES = {
    "last": (-1, RV_LAST, 0, lambda f: f.predict(single_shard=False) == (False, F.FINAL)),
    "layer": (1, RV_LAYER, 1, lambda f: f.predict(single_shard=False) == (False, F.LAYER) and F.FINAL in f.outcomes()),
    "first": (0, RV_FIRST, 0, lambda f: f.predict(single_shard=False) == (False, F.FINAL)),
}


def search_rv_deltas():
    m = Rv32(guests.commit_only(b"check me"))
    out = {}
    for name, (pos, cheats, final, want) in RV_CASES.items():
        i = pos % len(m.shards)
        out[name] = next((d for d in range(1, F.SEARCH_TRIES + 1) if want(m.forge(i, cheats(m.tallest(i), d), final=final)[1])), None)
    return out


def splice(words, forged):
    """the container with the payload of shard i replaced by forged[i] (same length: same shapes)"""
    w = words.copy()
    spans = _shard_spans(words)
    for i, b in forged.items():
        lo, hi = spans[i][1], spans[i][2]
        nw = np.frombuffer(b, np.uint32)
        assert len(nw) == hi - lo and (nw[:9] == words[lo:lo + 9]).all(), "a forged shard keeps its size and its main root"
        w[lo:hi] = nw
    return w


@pytest.fixture(scope="module")
def rv(prover):
    elf = guests.commit_only(b"check me")
    pk, vk = prover.setup(elf)
    proof, _ = prover.prove_core(pk, [])
    prover.pk_free(pk)
    words = np.frombuffer(proof, np.uint32).copy()
    model = Rv32(elf)
    assert len(_shard_spans(words)) == len(model.shards) == 5
    return vk, words, model


def _both(prover, vk, w):
    from dvt_circuits_amd import capi

    host = capi.verify(vk, w.tobytes(), Q, POW)
    dev = prover.verify(vk, w.tobytes(), Q, POW)
    assert dev == host, (dev, host)
    return host


def test_rv32_forged_last_shard(prover, rv):
    vk, words, m = rv
    n = len(m.shards)
    assert _both(prover, vk, words)[0]
    shard, f = m.forge(n - 1, RV_LAST(m.tallest(n - 1)))
    assert f.predict(single_shard=False) == (False, F.FINAL)
    host = _both(prover, vk, splice(words, {n - 1: shard}))
    assert not host[0] and host[3] == "shard %d: %s" % (n, F.FINAL)
    assert _both(prover, vk, words)[0]


def test_rv32_two_forged_shards_report_the_first(prover, rv):
    vk, words, m = rv
    s2, f2 = m.forge(1, RV_LAYER(m.tallest(1)), final=1)
    s3, f3 = m.forge(2, [F.final_poly(1)])
    assert f2.predict(single_shard=False) == (False, F.LAYER) and f3.predict(single_shard=False) == (False, F.FINAL)
    assert F.FINAL in f2.outcomes()       # (a later query of shard 2 fails the other way)
    host = _both(prover, vk, splice(words, {1: s2, 2: s3}))
    assert not host[0] and host[3] == "shard 2: " + F.LAYER
    host = _both(prover, vk, splice(words, {2: s3}))
    assert not host[0] and host[3] == "shard 3: " + F.FINAL


def test_rv32_query_failure_of_shard_1_comes_before_host_failure_of_shard_2(prover, rv):
    vk, words, m = rv
    s1, f1 = m.forge(0, RV_FIRST(m.tallest(0)))
    assert f1.predict(single_shard=False) == (False, F.FINAL)
    w = splice(words, {0: s1})
    at = _shard_spans(words)[1][1] + 17      # the first word of shard 2's quotient root: its host part fails, no header changes
    w[at] = (int(w[at]) + 1) % P
    host = _both(prover, vk, w)
    assert not host[0] and host[3] == "shard 1: " + F.FINAL
    alone = words.copy()
    alone[at] = w[at]
    host = _both(prover, vk, alone)
    assert not host[0] and host[3].startswith("shard 2: ") and "Merkle" not in host[3] and F.FINAL not in host[3]


# ---------------------------------------------------------------- chunking
def test_three_chunks_give_the_same_answers(prover, rv):
    from dvt_circuits_amd import capi

    vk, words, m = rv
    spans = _shard_spans(words)
    n = len(spans)
    biggest = max(hi - lo for _, lo, hi in spans)
    # a chunk holds the key's prep root (8 words) and shards.  At 8 + the largest shard every shard fits, and no two do:
    # a second shard is added only while 8 + n1 + n2 <= 8 + max(n), which no two positive sizes meet
    small = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": 10, "verify_chunk_words": %d}' % (Q, POW, biggest + 8))
    try:
        honest = small.verify(vk, words.tobytes(), Q, POW)
        t = small.verify_times()
        print("chunked verify:", t)
        assert honest == prover.verify(vk, words.tobytes(), Q, POW) and honest[0]
        assert t["chunks"] == n >= 3 and t["launches"] == 4 * t["chunks"]
        assert prover.verify_times()["chunks"] == 1
        # the last shard is the fifth chunk: slot 0 used for the third time
        shard, f = m.forge(n - 1, RV_LAST(m.tallest(n - 1)))
        w = splice(words, {n - 1: shard}).tobytes()
        got = small.verify(vk, w, Q, POW)
        assert got == prover.verify(vk, w, Q, POW) == capi.verify(vk, w, Q, POW)
        assert not got[0] and got[3] == "shard %d: %s" % (n, F.FINAL)
        # a forged middle shard: its chunk is in flight while the next one is flattened
        s2, _ = m.forge(1, RV_LAYER(m.tallest(1)), final=1)
        w = splice(words, {1: s2}).tobytes()
        got = small.verify(vk, w, Q, POW)
        assert got == capi.verify(vk, w, Q, POW) and got[3] == "shard 2: " + F.LAYER
        assert small.verify(vk, words.tobytes(), Q, POW) == honest
    finally:
        small.close()


def test_a_shard_larger_than_the_chunk_goes_alone(prover, rv):
    from dvt_circuits_amd import capi

    vk, words, m = rv
    one = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "verify_chunk_words": 1}' % (Q, POW))
    try:
        assert one.verify(vk, words.tobytes(), Q, POW) == prover.verify(vk, words.tobytes(), Q, POW)
        assert one.verify_times()["chunks"] == len(m.shards)
    finally:
        one.close()


@pytest.mark.parametrize("value", [0, -1])
def test_verify_chunk_words_must_be_positive(value):
    from dvt_circuits_amd import capi

    with pytest.raises(capi.DvtError) as e:
        capi.Prover('{"verify_chunk_words": %d}' % value)
    assert e.value.code == capi.DVT_ERR_INPUT and "verify_chunk_words" in e.value.msg


if __name__ == "__main__":
    print(search_rv_deltas())
