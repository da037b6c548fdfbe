"""GPU tests of the reference boundary on the rv32 machine: setup(elf) ->
prove_core(stdin) -> verify, through the C-ABI (reference src/main.rs:461-474),
single- and multi-shard."""
import struct

import numpy as np
import pytest

from tests import guests

pytestmark = pytest.mark.gpu
Q, POW = 24, 8


def cfg(log_shard=21):
    return '{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d}' % (Q, POW, log_shard)


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available()
    p = capi.Prover(cfg())
    yield p
    p.close()


def test_arith_guest_proof_verifies(gpu):
    from dvt_circuits_amd import capi

    elf, want = guests.arith()
    pk, vk = gpu.setup(elf)
    proof, rep = gpu.prove_core(pk)
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok, why
    assert ec == 0 and pv == guests.checksum(want) and rep["exit_code"] == 0
    # same input -> same proof bytes
    assert gpu.prove_core(pk)[0] == proof
    # tampering anywhere is rejected: container header, the public-value bytes (bound through the COMMITted
    # words of their SHA-256 digest, whose receiving side the verifier supplies), and the shard proofs
    words = np.frombuffer(proof, dtype=np.uint32).copy()
    rng = np.random.default_rng(3)
    body = len(words) - sum(1 + len(s) // 4 for s in capi.split_container(proof)[2])   # the first shard's length word
    for pos in [1, 2, 3, 4, 5, body - 1, body, body + 1] + list(rng.integers(4, len(words), 20)):
        w = words.copy()
        w[pos] = (int(w[pos]) + 1) % 2013265921
        assert not capi.verify(vk, w.tobytes(), Q, POW)[0], f"tampered word {pos} accepted"
    # a key for a different program must reject the proof
    pk2, vk2 = gpu.setup(guests.bignum(1, limbs=2)[0])
    assert not capi.verify(vk2, proof, Q, POW)[0]
    gpu.pk_free(pk)
    gpu.pk_free(pk2)


def test_bignum_and_hint_guests(gpu):
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(20, limbs=12)
    pk, vk = gpu.setup(elf)
    proof, rep = gpu.prove_core(pk)
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and pv == want, why
    assert rep["cycles"] > 40000
    gpu.pk_free(pk)

    elf = guests.hint_sum()
    pk, vk = gpu.setup(elf)
    data = struct.pack("<16I", *range(1, 17))
    proof, _ = gpu.prove_core(pk, [data])
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and struct.unpack("<I", pv)[0] == 136, why
    gpu.pk_free(pk)


@pytest.mark.parametrize("which", ["subword", "shifts", "muldiv", "sha_extend", "sha256_precompiled"])
def test_subword_and_shift_guest_proofs(gpu, which):
    from dvt_circuits_amd import capi

    elf, want = getattr(guests, which)()
    pk, vk = gpu.setup(elf)
    proof, rep = gpu.prove_core(pk)
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and pv == guests.checksum(want), why
    gpu.pk_free(pk)


def test_multi_shard_proof(gpu):
    """one execution cut into 2^10-cycle shards: the shards verify only together (common LogUp
    challenges, memory bus balanced across shards, pc / shard-index chaining)"""
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(3, limbs=12)          # ~7k cycles of arithmetic + ~11k of the SHA-256 exit path -> 18 shards
    p = capi.Prover(cfg(10))
    pk, vk = p.setup(elf)
    proof, rep = p.prove_core(pk)
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and pv == want, why
    w = np.frombuffer(proof, np.uint32)
    n = int(w[1])
    assert n == (rep["cycles"] + 1023) // 1024 and n > 4
    # the shard-level API (what the multi-GPU bench uses) assembles the same bytes
    job, _ = p.prepare(pk)
    headers = [p.commit_shard(pk, job, i) for i in range(n)]
    ch = capi.rv32_challenges(vk, headers)
    shard_proofs = [p.prove_shard(pk, job, i, ch) for i in range(n)]
    assert p.assemble(job, shard_proofs) == proof
    # dropping, swapping or replaying a shard must be rejected
    assert not capi.verify(vk, p.assemble(job, shard_proofs[:1] + shard_proofs[2:] + shard_proofs[1:2]), Q, POW)[0]
    shards = capi.split_container(proof)[2]
    at = len(w) - sum(1 + len(s) // 4 for s in shards)   # the first shard's length word
    first_len = len(shards[0]) // 4
    truncated = w.copy()
    truncated[1] = n - 1
    cut = np.concatenate([truncated[:at], truncated[at + 1 + first_len:]])
    assert not capi.verify(vk, cut.tobytes(), Q, POW)[0]
    # a shard proven under different challenges does not fit
    bad = p.prove_shard(pk, job, 1, (ch + 1) % 2013265921)
    assert not capi.verify(vk, p.assemble(job, [shard_proofs[0], bad] + shard_proofs[2:]), Q, POW)[0]
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_full_size_shard_on_the_reference_input():
    """BASELINE configs[1] at full size: the reference's finalization example through its host encoding, one shard
    of ~2^21 cycles, production parameters (100 queries, 16 PoW bits).  No CPU oracle at this size: the properties are
    acceptance by the verifier with the public values the guest must commit, determinism, and rejection of a tampered word."""
    import os

    from dvt_circuits_amd import capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tests", "golden", "finalization_example.json"), "rb") as f:
        buf = capi.stdin_from_json("finalization", f.read())
    elf, want = guests.finalization_like(899, buf)
    p = capi.Prover("{}")
    pk, vk = p.setup(elf)
    proof, rep = p.prove_core(pk, [buf])
    assert (1 << 21) - 4096 < rep["cycles"] <= 1 << 21
    w = np.frombuffer(proof, np.uint32)
    assert int(w[1]) == 1                                     # one shard
    ok, ec, pv, why = capi.verify(vk, proof)
    assert ok and ec == 0 and pv == want, why
    assert p.prove_core(pk, [buf])[0] == proof
    for pos in (len(w) // 3, len(w) // 2, len(w) - 5):
        t = w.copy()
        t[pos] = (int(t[pos]) + 1) % 2013265921
        assert not capi.verify(vk, t.tobytes())[0]
    # a different input of the same length changes the committed values, and the old proof's values no longer match it
    other = bytearray(buf)
    other[100] ^= 1
    proof2, _ = p.prove_core(pk, [bytes(other)])
    ok2, _, pv2, _ = capi.verify(vk, proof2)
    assert ok2 and pv2 != pv and pv2 == guests.finalization_like(899, bytes(other))[1]
    p.pk_free(pk)
    p.close()


def test_phase2_recompute_path_gives_the_same_bytes(gpu):
    """with "keep_phase1": 0 (what a GPU short of HBM falls back to) phase 2 regenerates the traces and the main
    commitment of every shard: same proof, byte for byte"""
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(3, limbs=12)
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": 10}' % (Q, POW))
    pk, vk = p.setup(elf)
    kept, _ = p.prove_core(pk)
    p.pk_free(pk)
    p.close()
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": 10, "keep_phase1": 0}' % (Q, POW))
    pk, vk2 = p.setup(elf)
    recomputed, _ = p.prove_core(pk)
    assert vk2 == vk and recomputed == kept
    ok, ec, pv, why = capi.verify(vk, recomputed, Q, POW)
    assert ok and pv == want, why
    p.pk_free(pk)
    p.close()


def test_guest_without_the_commit_epilogue_is_refused(gpu):
    """a guest that halts without COMMITting the SHA-256 digest of its public values could only yield a proof the
    verifier rejects (the verifier supplies the receiving side of the public-values bus): prove refuses it up front"""
    from dvt_circuits_amd import capi

    pk, _ = gpu.setup(guests.arith(commit=False)[0])
    with pytest.raises(capi.DvtError) as e:
        gpu.prove_core(pk)
    assert e.value.code == capi.DVT_ERR_GUEST and "COMMIT" in str(e.value)
    gpu.pk_free(pk)


def test_verify_rejects_hostile_containers(gpu):
    """a crafted chip id used to index a stack array before any range check; parameter floors"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"abcd")
    pk, vk = gpu.setup(elf)
    proof, _ = gpu.prove_core(pk)
    assert capi.verify(vk, proof, Q, POW)[0]
    w = np.frombuffer(proof, np.uint32).copy()
    # word layout: magic, n, exit code, pv length, pv words, shard length, then the shard proof: magic, 3 roots (24), pubs (1 + 5),
    # chip count, first chip id
    at = 4 + 1 + 1 + 1 + 24 + 6 + 1
    assert w[at] == 0 and w[at - 1] in (5, 6)         # program chip first; 5 or 6 chips present
    for evil in (0xFFFFFFFF, 64, 7):
        t = w.copy()
        t[at] = evil
        assert not capi.verify(vk, t.tobytes(), Q, POW)[0]
    for q, pw in ((0, POW), (Q, 31), (Q, 40), (5000, POW)):
        ok, _, _, why = capi.verify(vk, proof, q, pw)
        assert not ok
    # the container's exit-code word is compared mod p with the proven public value; ec + p must not be
    # accepted (and then reported to the caller as the exit code)
    assert w[2] == 0
    for evil in (2013265921, 1 << 24, 0xF0000002):
        t = w.copy()
        t[2] = evil
        ok, _, _, why = capi.verify(vk, t.tobytes(), Q, POW)
        assert not ok and "exit code" in why, why
    gpu.pk_free(pk)


def test_error_classes(gpu):
    from dvt_circuits_amd import capi

    pk, _ = gpu.setup(guests.exit_with(3))
    with pytest.raises(capi.DvtError) as e:
        gpu.prove_core(pk)
    assert e.value.code == capi.DVT_ERR_GUEST
    gpu.pk_free(pk)
    pk, _ = gpu.setup(guests.uses_unprovable())
    with pytest.raises(capi.DvtError) as e:
        gpu.prove_core(pk)
    assert e.value.code == capi.DVT_ERR_UNSUPPORTED
    gpu.pk_free(pk)
    with pytest.raises(capi.DvtError) as e:
        gpu.setup(b"\x7fELF garbage")
    assert e.value.code == capi.DVT_ERR_INPUT


def test_reference_horner_kat_is_proven_through_the_curve_precompiles(gpu):
    """reference crates/dkg/src/dkg_math.rs:281-300: evaluate_polynomial of three public keys at id 1.  The guest decompresses
    the keys (with the subgroup check), evaluates through the BLS12381 precompile chips and commits the compressed result:
    the PROVEN public values are the reference's known answer."""
    from dvt_circuits_amd import capi
    from tests import guests_bls, test_guest_bls_horner as th

    pks = [bytes.fromhex(h) for h in th.HORNER_PKS]
    elf = guests_bls.horner(pks, [1, 2], subgroup_check=True)
    pk, vk = gpu.setup(elf)
    proof, rep = gpu.prove_core(pk)
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and ec == 0, why
    assert pv[:48].hex() == th.HORNER_TARGET and pv == th.expected_horner(pks, [1, 2])
    # a different claimed result is rejected
    w = np.frombuffer(proof, np.uint32).copy()
    w[4] ^= 1
    assert not capi.verify(vk, w.tobytes(), Q, POW)[0]
    gpu.pk_free(pk)


def test_reference_finalization_example_is_proven_with_the_reference_public_values(gpu):
    """BASELINE configs[1]: finalization_prove on examples/finalization_test.json.  The re-stated guest
    (tests/guests_finalization.py: everything of crates/finalization_prove/src/main.rs but the pairings) is executed AND
    proven on the reference's own example input; the proof verifies and its public values are the bytes the reference
    commits (main.rs:26-32)."""
    import json
    import os

    from dvt_circuits_amd import capi
    from tests import guests_finalization as gf

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    example = open(os.path.join(root, "tests", "golden", "finalization_example.json"), "rb").read()
    buf = capi.stdin_from_json("finalization", example)
    elf = gf.finalization(nmax=8, kmax=8)
    pk, vk = gpu.setup(elf)
    proof, rep = gpu.prove_core(pk, [buf])
    ok, ec, pv, why = capi.verify(vk, proof, Q, POW)
    assert ok and ec == 0, why
    assert pv == gf.expected_public_values(json.loads(example)) and len(pv) == 320
    # a vector the reference expects to FAIL (wrong aggregate key) cannot be proven: the guest halts with exit code 1
    vec = json.load(open(os.path.join(root, "tests", "golden", "finalization_vectors", "report-1-wrong-aggregate-pubkey.json")))
    bad = capi.stdin_from_json("finalization", json.dumps(vec["scenario"]).encode())
    with pytest.raises(capi.DvtError) as e:
        gpu.prove_core(pk, [bad])
    assert e.value.code == capi.DVT_ERR_GUEST
    gpu.pk_free(pk)
