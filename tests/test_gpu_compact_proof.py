"""GPU tests of the compact proof form ("DVP2"): the tree kernel of the device verifier through its stage hook
(dvt_stage_verify_multipath) on trees built with the oracle's compression, the prover's "compact_openings" against
dvt_proof_compact of the default prover's bytes, and host / device agreement on honest, forged and mixed containers.

Shapes of the stage test: depths 0, 1, 2, 5 and 12 with 1, 2, 17, 100 and 300 queries: more queries than leaves, more jobs
on a level than the 16 rows of one pass of the workgroup, and levels that shrink to one job."""
import numpy as np
import pytest

from tests import _compact
from tests import _forger as F
from tests import _orc, guests, toy_traces

pytestmark = pytest.mark.gpu
Q, POW = F.Q, F.POW
P = F.P


@pytest.fixture(scope="module")
def prover():
    from dvt_circuits_amd import capi

    p = capi.Prover({"fri_queries": Q, "pow_bits": POW, "log_shard_size": 10})
    yield p
    p.close()


@pytest.fixture(scope="module")
def compact_prover():
    from dvt_circuits_amd import capi

    p = capi.Prover({"fri_queries": Q, "pow_bits": POW, "log_shard_size": 10, "compact_openings": 1})
    yield p
    p.close()


# ---------------------------------------------------------------- the tree kernel
INJECT = {"none": lambda d: None, "top": lambda d: [lh == 0 for lh in range(d)], "middle": lambda d: [lh == d // 2 for lh in range(d)],
          "leaves": lambda d: [lh == d - 1 for lh in range(d)], "all": lambda d: [True] * d}


@pytest.fixture(scope="module")
def trees():
    oracle = _orc.load()
    rng = np.random.default_rng(12)
    out = {(d, k): _compact.Tree(oracle, rng, d, INJECT[k](d)) for d in (0, 1, 2, 5, 12) for k in (("none", "all") if d == 12 else INJECT)
           if d or k == "none"}
    out[(10, "middle")] = _compact.Tree(oracle, rng, 10, INJECT["middle"](10))
    return out


@pytest.mark.parametrize("n", [1, 2, 17, 100, 300])
def test_tree_kernel_against_the_host_walk(prover, trees, n):
    rng = np.random.default_rng(100 + n)
    for (d, kind), tree in trees.items():
        if d == 10:
            continue    # (the tree of test_tree_kernel_at_the_cap_of_1024_queries)
        idx = [int(x) for x in rng.integers(0, 1 << 22, n)]
        if n >= 2:
            idx[1] = idx[0] ^ (1 << (d - 1)) if d else idx[0]   # both halves of a pair
        if n >= 17:
            idx[5] = idx[3]                                     # a repeated index
        leaf, inject, nodes = tree.opening(idx)
        at = tree.inject_at if kind != "none" else None

        def run(leaf=leaf, inject=inject, nodes=nodes, root=tree.root):
            return prover.verify_multipath(d, idx, leaf, nodes, root, inject if at is not None else None, at)

        assert len(nodes) == len(_compact.model_nodes(d, idx))
        assert run() is True, (d, kind, n)
        assert tree.walk(idx, leaf, inject, nodes, tree.root)

        def bump(a, pos):
            a = a.copy()
            a.reshape(-1)[pos] = (int(a.reshape(-1)[pos]) + 1) % P
            return a

        # any single listed node, leaf digest or joining digest (all of them on the small cases, 48 of each beyond)
        def some(count):
            return range(count) if count <= 48 else sorted(int(x) for x in rng.choice(count, 48, replace=False))

        for k in some(len(nodes)):
            assert run(nodes=bump(nodes, 8 * k + k % 8)) is False, (d, kind, n, "node", k)
        for q in some(n):
            assert run(leaf=bump(leaf, 8 * q + q % 8)) is False, (d, kind, n, "leaf", q)
        if at is not None:
            for lh in np.flatnonzero(at):
                for q in some(n):
                    assert run(inject=bump(inject, 8 * (int(lh) * n + q) + q % 8)) is False, (d, kind, n, "inject", lh, q)
        assert run(root=bump(tree.root, 3)) is False
        # the same answers as the host walk, on one tampered input of each kind
        if len(nodes):
            assert not tree.walk(idx, leaf, inject, bump(nodes, 8 * (len(nodes) - 1)), tree.root)
        assert not tree.walk(idx, bump(leaf, 8 * (n - 1)), inject, nodes, tree.root)


@pytest.mark.parametrize("key", [(10, "middle"), (12, "all")])
def test_tree_kernel_at_the_cap_of_1024_queries(prover, trees, key):
    """1024 distinct leaves: both LDS buffers full (2 x 1024 x 32 B = 64 KB, the most a launch gets without a function
    attribute), 64 passes of the 16 rows on the first level.  Depth 10: every leaf queried, nothing listed; depth 12: a
    quarter of the leaves."""
    d = key[0]
    tree = trees[key]
    rng = np.random.default_rng(7)
    idx = [int(x) for x in rng.permutation(1 << d)[:1024]]
    leaf, inject, nodes = tree.opening(idx)
    assert len(set(i % (1 << d) for i in idx)) == 1024 and (len(nodes) == 0) == (d == 10)

    def run(leaf=leaf, inject=inject, nodes=nodes):
        return prover.verify_multipath(d, idx, leaf, nodes, tree.root, inject, tree.inject_at)

    def bump(a, pos):
        a = a.copy()
        a.reshape(-1)[pos] = (int(a.reshape(-1)[pos]) + 1) % P
        return a

    assert run() is True
    for q in (0, 15, 16, 511, 1008, 1023):                    # first and last rows of the first and last pass
        assert run(leaf=bump(leaf, 8 * q + q % 8)) is False, q
    lh = int(np.flatnonzero(tree.inject_at)[0])
    assert run(inject=bump(inject, 8 * (lh * 1024 + 1023))) is False
    for k in ([0, len(nodes) // 2, len(nodes) - 1] if len(nodes) else []):
        assert run(nodes=bump(nodes, 8 * k + 7)) is False, k
    # one query more is refused before anything is launched
    from dvt_circuits_amd import capi

    with pytest.raises(capi.DvtError) as e:
        prover.verify_multipath(d, idx + [idx[0]], np.concatenate([leaf, leaf[:1]]), nodes, tree.root)
    assert e.value.code == capi.DVT_ERR_INPUT


def test_a_wrong_node_count_is_an_input_error(prover, trees):
    from dvt_circuits_amd import capi

    tree = trees[(5, "none")]
    leaf, inject, nodes = tree.opening([3, 9])
    with pytest.raises(capi.DvtError) as e:
        prover.verify_multipath(5, [3, 9], leaf, nodes[:-1], tree.root)
    assert e.value.code == capi.DVT_ERR_INPUT


# ---------------------------------------------------------------- the toy machine
@pytest.mark.parametrize("shape", [F.BIG, F.SMALL])
def test_toy_compact_prover_equals_the_transcoder(prover, compact_prover, shape):
    from dvt_circuits_amd import capi

    prep, main, pubs = toy_traces.build(*shape)
    pk, vk = prover.machine_setup("toy", prep)
    plain = prover.machine_prove(pk, main, pubs)
    prover.pk_free(pk)
    pk2, vk2 = compact_prover.machine_setup("toy", prep)
    comp = compact_prover.machine_prove(pk2, main, pubs)
    compact_prover.pk_free(pk2)
    assert vk2 == vk
    assert comp == capi.proof_compact(vk, plain, Q, POW) and len(comp) < len(plain)
    assert capi.proof_expand(vk, comp, Q, POW) == plain
    assert capi.machine_verify(vk, comp, Q, POW) == (True, "") == prover.machine_verify(vk, comp, Q, POW)
    w = np.frombuffer(comp, np.uint32).copy()
    lay = _compact.shard_layout(w)
    for cnt, a, b in lay["lists"]:
        if b > a:
            t = _compact.bump(w, a).tobytes()
            host = capi.machine_verify(vk, t, Q, POW)
            assert not host[0] and host == prover.machine_verify(vk, t, Q, POW), host


def test_the_default_prover_writes_the_plain_form(prover):
    """The flag is off by default: a handle without the key and an unconfigured one write the same DVP1 bytes.  (That these
    are the bytes from before the compact form existed is what the oracle parity tests and smoke() pin, not this test.)"""
    from dvt_circuits_amd import capi

    prep, main, pubs = toy_traces.build(*F.SMALL)
    other = capi.Prover('{"fri_queries": %d, "pow_bits": %d}' % (Q, POW))
    try:
        pk, vk = prover.machine_setup("toy", prep)
        pk2, _ = other.machine_setup("toy", prep)
        a, b = prover.machine_prove(pk, main, pubs), other.machine_prove(pk2, main, pubs)
        prover.pk_free(pk)
        other.pk_free(pk2)
    finally:
        other.close()
    assert a == b and np.frombuffer(a, np.uint32)[0] == _compact.DVP1


@pytest.mark.parametrize("c", F.CASES, ids=[c["name"] for c in F.CASES])
def test_compacted_toy_forgeries_host_and_device_agree(prover, c):
    from dvt_circuits_amd import capi

    proof, prep_root, f = F.forge_case(c)
    vk = F.toy_vk(prep_root)
    plain = capi.machine_verify(vk, proof, c["q"], POW)
    try:
        comp = capi.proof_compact(vk, proof, c["q"], POW)
    except capi.DvtError as e:
        # a forgery the host part refuses (a cumulative sum, the witness) is refused by the transcoder with the same text
        assert e.code == capi.DVT_ERR_REJECTED and plain == (False, e.msg), (e.code, e.msg, plain)
        return
    host = capi.machine_verify(vk, comp, c["q"], POW)
    dev = prover.machine_verify(vk, comp, c["q"], POW)
    assert dev == host, (dev, host)
    assert host[0] == plain[0]
    # the compact form checks tree by tree: a layer failure of any query is named before a final-value failure
    if not plain[0] and F.LAYER in f.outcomes():
        assert host[1] == F.LAYER, (host, plain)
    elif not plain[0]:
        assert host[1] == plain[1], (host, plain)


# ---------------------------------------------------------------- rv32
@pytest.fixture(scope="module")
def rv(prover, compact_prover):
    out = {}
    for name, elf in (("commit", guests.commit_only(b"check me")), ("curve", guests.curve_ops()[0])):
        pk, vk = prover.setup(elf)
        plain, _ = prover.prove_core(pk, [])
        prover.pk_free(pk)
        pk2, vk2 = compact_prover.setup(elf)
        comp, _ = compact_prover.prove_core(pk2, [])
        compact_prover.pk_free(pk2)
        assert vk == vk2
        out[name] = (vk, plain, comp)
    return out


@pytest.mark.parametrize("name", ["commit", "curve"])
def test_rv32_compact_prover_equals_the_transcoder(prover, rv, name):
    from dvt_circuits_amd import capi

    vk, plain, comp = rv[name]
    assert comp == capi.proof_compact(vk, plain, Q, POW)
    assert capi.proof_expand(vk, comp, Q, POW) == plain
    print(f"{name}: plain {len(plain)} bytes, compact {len(comp)} bytes, ratio {len(comp) / len(plain):.3f}")
    host = capi.verify(vk, comp, Q, POW)
    assert host[0] and host == prover.verify(vk, comp, Q, POW) == capi.verify(vk, plain, Q, POW)
    t = prover.verify_times()
    assert t["launches"] == 4 * t["chunks"]      # reduced openings, folds, sponges, trees: no path kernel


def test_rv32_mixed_and_tampered_containers(prover, rv):
    from dvt_circuits_amd import capi

    vk, plain, comp = rv["commit"]
    head, ps = _compact.container_parts(plain)
    _, cs = _compact.container_parts(comp)
    n = len(ps)
    assert n >= 3
    mixed = [ps[0]] + cs[1:-1] + [ps[-1]]
    good = _compact.container_join(head, mixed)
    assert capi.verify(vk, good, Q, POW) == prover.verify(vk, good, Q, POW) and capi.verify(vk, good, Q, POW)[0]
    assert prover.verify_times()["launches"] == 5   # one chunk holds chains and trees
    lay = _compact.shard_layout(cs[1])
    tree2, layer0 = lay["lists"][2], lay["lists"][4]
    small = capi.Prover({"fri_queries": Q, "pow_bits": POW, "verify_chunk_words": max(len(s) for s in mixed) + 8})
    try:
        for positions, want in (([tree2[1]], "shard 2: Merkle opening rejected (input tree)"), ([layer0[1]], "shard 2: " + F.LAYER),
                                ([tree2[2] - 1, layer0[1]], "shard 2: Merkle opening rejected (input tree)"),
                                ([lay["queries_end"] - 1], None)):
            t = cs[1]
            for pos in positions:
                t = _compact.bump(t, pos)
            bad = _compact.container_join(head, [ps[0], t] + mixed[2:])
            host = capi.verify(vk, bad, Q, POW)
            assert not host[0] and (want is None or host[3] == want), host
            assert prover.verify(vk, bad, Q, POW) == host
            # one chunk per shard: two slots in flight, slot 0 reused
            assert small.verify(vk, bad, Q, POW) == host
            assert small.verify_times()["chunks"] == n
        assert small.verify(vk, good, Q, POW) == capi.verify(vk, good, Q, POW)
        # a count that does not match the indices is answered on the host, with the host's text
        t = cs[1].copy()
        t[tree2[0]] -= 1
        t[lay["lists"][3][0]] += 1
        t = np.concatenate([t[:tree2[2] - 8], [t[lay["lists"][3][0]]], t[tree2[2] - 8:tree2[2]], t[lay["lists"][3][0] + 1:]]).astype(np.uint32)
        bad = _compact.container_join(head, [ps[0], t] + mixed[2:])
        host = capi.verify(vk, bad, Q, POW)
        assert not host[0] and "node list length" in host[3] and prover.verify(vk, bad, Q, POW) == host
    finally:
        small.close()


def test_hundred_queries_on_small_shards():
    from dvt_circuits_amd import capi

    q, pw = 100, 16
    elf = guests.commit_only(b"check me")    # between 2^12 and 2^12 + 2^10 cycles: two shards
    out = []
    for compact in (0, 1):
        p = capi.Prover({"fri_queries": q, "pow_bits": pw, "log_shard_size": 12, "compact_openings": compact})
        try:
            pk, vk = p.setup(elf)
            proof, rep = p.prove_core(pk, [])
            p.pk_free(pk)
            host = capi.verify(vk, proof, q, pw)
            assert host[0] and p.verify(vk, proof, q, pw) == host
            out.append((vk, proof, p.verify_times()))
        finally:
            p.close()
    (vk, plain, t0), (_, comp, t1) = out
    assert len(_compact.container_parts(plain)[1]) >= 2
    assert capi.proof_compact(vk, plain, q, pw) == comp and capi.proof_expand(vk, comp, q, pw) == plain
    print(f"100 queries: plain {len(plain)} bytes, compact {len(comp)} bytes, ratio {len(comp) / len(plain):.3f}")
    print("verify_times plain:", t0, "compact:", t1)
    assert t1["permutations"] < t0["permutations"]
