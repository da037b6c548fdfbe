"""CPU tests of the compact proof form ("DVP2": shared Merkle paths sent once) on the committed GPU-made proofs
(tests/golden/proof_*.bin, 4 FRI queries, 4 PoW bits): dvt_proof_compact, dvt_proof_expand and the host verifier need no
device.  The node rule itself is pinned against a Python model (tests/_compact.py)."""
import os
import struct

import numpy as np
import pytest

from dvt_circuits_amd import capi
from tests import _compact, guests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, POW = 4, 4


def _load(name):
    blob = open(os.path.join(ROOT, "tests", "golden", f"proof_{name}.bin"), "rb").read()
    (n,) = struct.unpack_from("<I", blob)
    vk, proof = blob[4:4 + n], blob[4 + n:]
    assert capi.verify(vk, proof, Q, POW)[0], "stale fixture: regenerate with tools/make_proof_fixture.py on a GPU box"
    return vk, proof


@pytest.fixture(scope="module", params=["commit", "curve"])
def fx(request):
    vk, proof = _load(request.param)
    return request.param, vk, proof, capi.proof_compact(vk, proof, Q, POW)


def test_compact_verifies_and_round_trips(fx):
    name, vk, proof, comp = fx
    want = b"fuzz me!" if name == "commit" else guests.checksum(guests.curve_ops()[1])
    ok, ec, pv, why = capi.verify(vk, comp, Q, POW)
    assert ok and (ec, pv) == (0, want), why
    assert (ok, ec, pv) == capi.verify(vk, proof, Q, POW)[:3]
    assert len(comp) < len(proof)
    print(f"{name}: plain {len(proof)} bytes, compact {len(comp)} bytes, ratio {len(comp) / len(proof):.3f}")
    assert capi.proof_expand(vk, comp, Q, POW) == proof
    # either form comes back unchanged from the transcoder that makes it
    assert capi.proof_compact(vk, comp, Q, POW) == comp
    assert capi.proof_expand(vk, proof, Q, POW) == proof
    # every shard has its own magic, and nothing but the query section differs
    _, plain_shards = _compact.container_parts(proof)
    _, comp_shards = _compact.container_parts(comp)
    for a, b in zip(plain_shards, comp_shards):
        la, lb = _compact.shard_layout(a), _compact.shard_layout(b)
        assert not la["compact"] and lb["compact"] and la["head_end"] == lb["head_end"]
        assert np.array_equal(a[1:la["head_end"]], b[1:lb["head_end"]])
    # other parameters than the proof was made with are refused by the transcoders as by the verifier
    for fn in (capi.proof_compact, capi.proof_expand):
        with pytest.raises(capi.DvtError) as e:
            fn(vk, comp, Q + 1, POW)
        assert e.value.code == capi.DVT_ERR_REJECTED


def test_every_word_of_every_node_list_matters(fx):
    """Every word of every node list of every shard, changed by +1 mod p, is rejected.  A verify of these containers takes
    24 / 57 ms and their lists hold 23 824 / 34 456 words, so the whole sweep runs inside the library
    (dvt_debug_compact_list_sweep): the host part of a shard, which reads no node list, once per shard, and the walk of the
    list's tree once per changed word.  The public verifier is then given one changed word of EVERY listed digest of the
    first shard (the cheapest to refuse: the shards are verified in order), and a spread over the other shards."""
    name, vk, proof, comp = fx
    head, shards = _compact.container_parts(comp)
    words = np.frombuffer(comp, np.uint32).copy()
    in_lists = sum(b - a for s in shards for _, a, b in _compact.shard_layout(s)["lists"])
    n, accepted = capi.compact_list_sweep(vk, comp, Q, POW)
    assert n == in_lists > 20000 and accepted == 0, (n, in_lists, accepted)
    # a plain container has no list to sweep; one that does not verify is refused
    assert capi.compact_list_sweep(vk, proof, Q, POW) == (0, 0)
    with pytest.raises(capi.DvtError):
        capi.compact_list_sweep(vk, _compact.bump(words, len(words) - 1).tobytes(), Q, POW)
    rng = np.random.default_rng(11)
    base = len(head)
    for si, s in enumerate(shards):
        lay = _compact.shard_layout(s)
        start = base + 1
        if si == 0:
            picks = [a + 8 * k + (k % 8) for _, a, b in lay["lists"] for k in range((b - a) // 8)]
        else:
            inside = np.concatenate([np.arange(a, b) for _, a, b in lay["lists"]])
            picks = [int(x) for x in rng.choice(inside, 8, replace=False)]
        for pos in picks:
            ok, _, _, why = capi.verify(vk, _compact.bump(words, start + pos).tobytes(), Q, POW)
            assert not ok and "Merkle opening rejected" in why, (name, si, pos, why)
        base += 1 + len(s)


def test_tampered_counts_moved_nodes_and_other_words_are_rejected(fx):
    name, vk, proof, comp = fx
    head, shards = _compact.container_parts(comp)
    words = np.frombuffer(comp, np.uint32).copy()
    rng = np.random.default_rng(11)

    def rejected(w, what):
        ok, _, _, why = capi.verify(vk, np.asarray(w, np.uint32).tobytes(), Q, POW)
        assert not ok, f"{name}: {what} accepted"
        return why

    # a spread over the other words (field words + 1 mod p; counts / lengths + 1)
    for pos in list(range(0, 12)) + [int(x) for x in rng.integers(12, len(words), 120 if name == "commit" else 40)]:
        rejected(_compact.bump(words, pos), f"word {pos}")
    # a count off by one in either direction, and a node moved from one tree's list to the next
    s0, lay = shards[0], _compact.shard_layout(shards[0])
    for li, (cnt, a, b) in enumerate(lay["lists"]):
        for d in (1, -1):
            if d == -1 and s0[cnt] == 0:
                continue
            t = s0.copy()
            t[cnt] = int(t[cnt]) + d
            rejected(np.frombuffer(_compact.container_join(head, [t] + shards[1:]), np.uint32), f"list {li}: count {d:+d}")
        if li + 1 < len(lay["lists"]) and s0[cnt] > 0:
            nxt = lay["lists"][li + 1][0]
            # the last digest of list li becomes the first of list li + 1: the count word moves 8 words down
            t = np.concatenate([s0[:b - 8], [s0[nxt] + 1], s0[b - 8:b], s0[nxt + 1:]]).astype(np.uint32)
            t[cnt] = int(t[cnt]) - 1
            _compact.shard_layout(t)   # (still one well-formed stream)
            why = rejected(np.frombuffer(_compact.container_join(head, [t] + shards[1:]), np.uint32), f"list {li}: node moved")
            assert "node list length" in why, why
    # truncation and trailing words
    rejected(words[:-1], "truncated")
    rejected(words[:len(words) // 2], "half")
    rejected(np.concatenate([words, [0]]), "trailing word")
    t = np.concatenate([shards[-1], [0]]).astype(np.uint32)
    rejected(np.frombuffer(_compact.container_join(head, shards[:-1] + [t]), np.uint32), "trailing word in a shard")


def test_a_container_may_mix_the_two_forms(fx):
    name, vk, proof, comp = fx
    head, plain = _compact.container_parts(proof)
    _, comps = _compact.container_parts(comp)
    assert len(plain) >= 2
    mixed = _compact.container_join(head, [plain[0]] + comps[1:])
    assert capi.verify(vk, mixed, Q, POW)[:3] == capi.verify(vk, proof, Q, POW)[:3]
    mixed2 = _compact.container_join(head, [comps[0]] + plain[1:-1] + [comps[-1]])
    assert capi.verify(vk, mixed2, Q, POW)[0]
    # the transcoders take a mixed container to either pure form
    assert capi.proof_compact(vk, mixed, Q, POW) == comp and capi.proof_expand(vk, mixed2, Q, POW) == proof


def test_the_input_trees_are_reported_before_the_fri_layers(fx):
    name, vk, proof, comp = fx
    head, shards = _compact.container_parts(comp)
    lay = _compact.shard_layout(shards[0])
    tree2, layer0 = lay["lists"][2], lay["lists"][4]
    assert tree2[2] > tree2[1] and layer0[2] > layer0[1]

    def why_of(positions):
        t = shards[0]
        for pos in positions:
            t = _compact.bump(t, pos)
        ok, _, _, why = capi.verify(vk, _compact.container_join(head, [t] + shards[1:]), Q, POW)
        assert not ok
        return why

    assert why_of([layer0[1]]) == "shard 1: Merkle opening rejected (FRI layer)"
    assert why_of([tree2[1]]) == "shard 1: Merkle opening rejected (input tree)"
    assert why_of([tree2[1], layer0[1]]) == "shard 1: Merkle opening rejected (input tree)"
    # a changed FRI sibling changes the leaf of its layer: a layer failure, whatever the fold chain then ends in (the
    # final-value text needs consistent trees: the forged proofs of tests/test_gpu_compact_proof.py reach it)
    assert why_of([lay["queries_end"] - 4]) == "shard 1: Merkle opening rejected (FRI layer)"


def test_multipath_nodes_against_the_model():
    nodes = capi.multipath_nodes
    assert nodes(0, [0]) == nodes(0, [5, 9]) == []
    assert nodes(1, [0, 1]) == [] and nodes(1, [0]) == [(1, 1)] and nodes(1, [3]) == [(1, 0)]
    # one query: the plain path, from the leaf level upwards
    for depth, i in ((5, 19), (22, 0x2a5a5a), (10, 0)):
        path = [(s, (i % (1 << s)) ^ (1 << (s - 1))) for s in range(depth, 0, -1)]
        assert nodes(depth, [i]) == path == _compact.model_nodes(depth, [i])
    # every leaf queried: nothing to list; repeated indices count once; both halves of a pair
    assert nodes(6, list(range(64))) == []
    assert nodes(7, [3, 3, 3 + 128, 3]) == nodes(7, [3]) == _compact.model_nodes(7, [3])
    assert nodes(4, [2, 10]) == _compact.model_nodes(4, [2, 10]) == [(3, 6), (2, 0), (1, 1)]
    rng = np.random.default_rng(5)
    for depth in range(1, 23):
        for n in (1, 2, 3, 17, 100, 300):
            idx = [int(x) for x in rng.integers(0, 1 << 22, n)]
            got = nodes(depth, idx)
            assert got == _compact.model_nodes(depth, idx), (depth, n)
            assert len(got) <= n * depth
    # the issue's model figure: 100 queries on a tree of full height list about half of what 100 plain paths carry
    counts = [len(nodes(22, [int(x) for x in rng.integers(0, 1 << 22, 100)])) for _ in range(5)]
    assert all(0.6 * 2200 < c < 0.8 * 2200 for c in counts), counts
