"""Forged proofs against the host verifier (capi.machine_verify, no GPU): proofs of a dishonest prover
(tests/_forger.py: the oracle prover plus one deviation) whose transcript and Merkle trees are all consistent, so that the
verifier's decision is made where no flipped-word test reaches: the FRI fold chain and its final value, the layer leaves
the verifier derives itself, the cumulative sums, the zeta check and the proof of work.  For every case the verifier must
say what _forger.predict says from the forger's own data: the same decision and the same reason.

Each case's pattern (which query fails first, and how) is asserted, so a constant of _forger.DELTAS that has gone stale
fails here.  Measured on the host: the forger takes 0.25 s per toy proof (the Python challenger and ctypes calls of the
oracle prover; the cheats add nothing measurable), the 22 cases 6 s; an rv32 shard of 2^10 cycles (a 2^16-row byte
table), as tests/test_gpu_verify_forgeries.py forges them, takes 1.0 - 1.7 s."""
import pytest

from tests import _forger as F
from tests import _oracle_prover


def _honest(shape, q):
    chips, pubs = F.toy_chips(shape)
    return _oracle_prover.prove_shard("toy", chips, pubs, q, F.POW)


@pytest.fixture(scope="module")
def honest():
    return {shape: _honest(shape, F.Q) for shape in (F.BIG, F.SMALL)}


def test_python_built_key_accepts_the_honest_oracle_proof(honest):
    from dvt_circuits_amd import capi

    for shape, (proof, prep_root) in honest.items():
        vk = F.toy_vk(prep_root)
        assert capi.machine_verify(vk, proof, F.Q, F.POW) == (True, ""), shape
        # the same key and proof under another query count: the transcript no longer fits
        assert not capi.machine_verify(vk, proof, F.Q + 1, F.POW)[0]


def test_a_forgery_without_cheats_is_the_honest_proof(honest):
    proof, prep_root, f = F.forge_toy(F.BIG, [], F.Q, F.POW)
    assert (proof, prep_root) == honest[F.BIG]
    assert f.predict() == (True, "") and (f.last[0] == f.last[1]).all()


def test_every_required_pattern_has_a_case():
    have = {c["pattern"] for c in F.CASES}
    # (a), (b) twice, (c), (d), (e), (f), (g) and (h) of the coverage list
    assert {"final_at_0", "final_at_j", "final_at_last", "accepted", "layer", "final_then_layer", "layer_then_final", "final"} <= have
    names = [c["name"] for c in F.CASES]
    assert len(set(names)) == len(names) and set(names) == set(F.DELTAS)
    assert all(1 <= d <= F.SEARCH_TRIES for d in F.DELTAS.values())
    by = {c["name"]: c for c in F.CASES}
    assert by["c_accepted"]["q"] == 2
    assert any(n.startswith("g_") for n in names) and any(n.startswith("h_") for n in names)


@pytest.mark.parametrize("c", F.CASES, ids=[c["name"] for c in F.CASES])
def test_host_verifier_decides_like_the_prediction(c):
    from dvt_circuits_amd import capi

    proof, prep_root, f = F.forge_case(c)
    print(c["name"], "indices", f.idx, "outcomes", f.outcomes())
    assert F.PATTERNS[c["pattern"]](f), f"stale constant: {c['name']} no longer shows {c['pattern']}: {f.outcomes()}"
    want = f.predict()
    if c["name"] in F.HOST_REASONS:
        assert want == (F.HOST_REASONS[c["name"]] == "", F.HOST_REASONS[c["name"]])
    else:
        # the pattern pins the reason: the first failing query's
        assert want == ((False, F.first_failure(f)[1]) if any(f.outcomes()) else (True, ""))
    got = capi.machine_verify(F.toy_vk(prep_root), proof, c["q"], F.POW)
    assert got[0] == want[0], (got, want)
    if want[1].startswith(F.ZETA):
        assert got[1].startswith(want[1]), (got, want)     # (the reason names a chip)
    else:
        assert got[1] == want[1], (got, want)


def test_the_two_required_pairs_are_two_cheats_in_one_proof():
    by = {c["name"]: c for c in F.CASES}
    kinds = lambda n: sorted(x[0] for x in by[n]["cheats"](1))
    assert kinds("e_final_then_layer") == kinds("f_layer_then_final") == ["layer_value", "lde_point"]
    assert kinds("two_layers") == ["layer_value", "layer_value"]
    a, b = by["two_layers"]["cheats"](1)
    assert a[1] != b[1]


def test_lde_point_is_caught_by_exactly_the_queries_of_its_parity():
    """the expected behaviour of a single lde_point at k: rejected by the queries with idx & 1 == k & 1 (whatever the
    chip's height), and of a layer_value at k' of a layer of 2^lm values: "FRI layer" for idx = k' mod 2^lm, "final value"
    for the other queries of its parity"""
    by = {c["name"]: c for c in F.CASES}
    for name in ("a_quot_tall", "b_quot_tall_late", "h_quot_fib", "h_perm_pairs", "h_quot_one_row", "h_main_fib"):
        f = F.forge_case(by[name])[2]
        k = f.cheats[0][4]
        assert f.outcomes() == [F.FINAL if (i ^ k) & 1 == 0 else None for i in f.idx], name
    for name in ("d_layer_lm3", "d_layer_lm2"):
        f = F.forge_case(by[name])[2]
        _, layer, k, _ = f.cheats[0]
        size = 4 << (-layer - 1)
        assert f.outcomes() == [F.LAYER if i % size == k else F.FINAL if (i ^ k) & 1 == 0 else None for i in f.idx], name
