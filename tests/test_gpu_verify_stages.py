"""GPU tests of the device verifier's two hashing kernels through their stage hooks (dvt_stage_sponge_rows,
dvt_stage_verify_paths) against the oracle's Poseidon2, at the smallest shapes at which they can go wrong: sponge lengths
around the rate and its multiples, chain depths 0..22, and counts that leave the 16-lane rows and the waves ragged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2013265921
LENS = [1, 7, 8, 9, 15, 16, 17, 96, 1245]
COUNTS = [1, 3, 4, 5, 67]
DEPTHS = [0, 1, 2, 5, 22]


@pytest.fixture(scope="module")
def prover():
    from dvt_circuits_amd import capi

    p = capi.Prover('{"fri_queries": 4, "pow_bits": 4}')
    yield p
    p.close()


@pytest.fixture(scope="module")
def vectors(oracle):
    """one vector per length (words 0 and p - 1 included) with its oracle digest, computed once"""
    rng = np.random.default_rng(5)
    out = {}
    for n in LENS:
        v = rng.integers(0, P, n, dtype=np.uint32)
        v[0] = 0 if n % 2 else P - 1
        v[-1] = P - 1 if n % 2 else 0
        out[n] = (v, oracle.hash_slice(v))
    return out


@pytest.mark.parametrize("order", ["increasing", "decreasing"])
@pytest.mark.parametrize("n", COUNTS)
def test_sponges_equal_the_oracle(prover, vectors, n, order):
    lens = [LENS[i % len(LENS)] for i in range(n)] if n > 1 else [LENS[-1]]
    lens = sorted(lens, reverse=order == "decreasing")
    got = prover.stage_sponge_rows([vectors[k][0] for k in lens])
    for i, k in enumerate(lens):
        assert (got[i] == vectors[k][1]).all(), f"vector {i} of {k} words"


def test_every_length_alone(prover, vectors):
    for k in LENS:
        assert (prover.stage_sponge_rows([vectors[k][0]])[0] == vectors[k][1]).all(), k


def _chain(oracle, rng, depth, leaf, inject):
    """an honest chain; inject: 'none', 'all', 'leaf' (only the level below the leaves) or 'root' (only the last level)"""
    start = rng.integers(0, P, 8, dtype=np.uint32)
    sib = rng.integers(0, P, (depth, 8), dtype=np.uint32)
    at = np.zeros(depth, np.uint8)
    if depth:
        if inject == "all":
            at[:] = 1
        elif inject == "leaf":
            at[0] = 1
        elif inject == "root":
            at[-1] = 1
    inj = rng.integers(0, P, (depth, 8), dtype=np.uint32)
    cur, j = start, leaf & ((1 << depth) - 1)
    for l in range(depth):
        half = 1 << (depth - l - 1)
        cur = oracle.compress(cur, sib[l]) if j < half else oracle.compress(sib[l], cur)
        j &= half - 1
        if at[l]:
            cur = oracle.compress(cur, inj[l])
    c = dict(start=start, depth=depth, leaf=leaf, siblings=sib, root=cur)
    if inject != "none":
        c.update(inject=inj, inject_at=at)
    return c


@pytest.fixture(scope="module")
def chains(oracle):
    """67 honest chains: every depth with leaf 0, 2^d - 1 and random leaves, every injection pattern, depths mixed"""
    rng = np.random.default_rng(6)
    out = []
    kinds = ["none", "all", "leaf", "root"]
    for i in range(67):
        d = DEPTHS[i % len(DEPTHS)]
        leaf = [0, (1 << d) - 1, int(rng.integers(0, 1 << d))][(i // len(DEPTHS)) % 3]
        out.append(_chain(oracle, rng, d, leaf, kinds[(i // 3) % 4]))
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_honest_chains_are_accepted(prover, chains, n):
    pick = chains[-n:] if n < 67 else chains
    assert prover.stage_verify_paths(pick).tolist() == [1] * n
    if n > 1:   # depths in the other order inside the wave
        assert prover.stage_verify_paths(pick[::-1]).tolist() == [1] * n


def _bump(a, idx):
    a = np.array(a, np.uint32, copy=True)
    a.reshape(-1)[idx] = (int(a.reshape(-1)[idx]) + 1) % P
    return a


@pytest.mark.parametrize("what", ["sibling", "root", "start", "inject", "leaf"])
def test_one_changed_chain_fails_alone(prover, chains, what):
    rng = np.random.default_rng(7)
    for n in (5, 67):
        pick = [dict(c) for c in (chains[:n])]
        want = [1] * n
        if what == "inject":
            cands = [i for i, c in enumerate(pick) if c.get("inject") is not None and c["inject_at"].any()]
        elif what in ("sibling", "leaf"):
            cands = [i for i, c in enumerate(pick) if c["depth"] >= 1]
        else:
            cands = list(range(n))
        assert cands
        for victim in {cands[0], cands[-1], cands[len(cands) // 2]}:
            bad = [dict(c) for c in pick]
            c = bad[victim]
            if what == "sibling":
                c["siblings"] = _bump(c["siblings"], int(rng.integers(0, c["siblings"].size)))
            elif what == "root":
                c["root"] = _bump(c["root"], int(rng.integers(0, 8)))
            elif what == "start":
                c["start"] = _bump(c["start"], int(rng.integers(0, 8)))
            elif what == "inject":
                l = int(np.flatnonzero(c["inject_at"])[-1])
                c["inject"] = _bump(c["inject"], 8 * l + int(rng.integers(0, 8)))
            else:
                c["leaf"] = c["leaf"] ^ (1 << int(rng.integers(0, c["depth"])))
            exp = list(want)
            exp[victim] = 0
            assert prover.stage_verify_paths(bad).tolist() == exp, (what, n, victim, c["depth"])
