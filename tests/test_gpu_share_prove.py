"""GPU tests of the reference's bad-share statement (tests/guests_share.py, reference crates/bad_share_exchange_prove): the
slashable vectors of the reference (tests/golden/share_vectors/) are proven at the default configuration and verified with
the public values of the Python restatement (tools/dkg_verify.verify_share); a valid share cannot be proven; the shard
proofs equal the oracle CPU prover's byte for byte; the host CLI proves and verifies a vector end to end."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from tests import _oracle_prover, guests_share as gs
from tools import dkg_verify

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = os.path.join(ROOT, "tests", "golden", "share_vectors")
CLI = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")
SLASHABLE = ["seeds-commitment-from-2-to-1-bad-base-hash.json", "seeds-commitment-from-2-to-1-bad-dst-base-hash.json",
             "seeds-commitment-from-2-to-1-bad-secret-key.json"]
BABYBEAR = 2013265921


def vector(name):
    from dvt_circuits_amd import capi

    scenario = json.load(open(os.path.join(VECTORS, name)))["scenario"]
    return scenario, capi.stdin_from_json("bad-share", json.dumps(scenario).encode())


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available()
    p = capi.Prover("{}")                    # the default configuration
    yield p
    p.close()


@pytest.fixture(scope="module")
def keys(gpu):
    pk, vk = gpu.setup(gs.bad_share())
    yield pk, vk
    gpu.pk_free(pk)


@pytest.mark.parametrize("name", SLASHABLE)
def test_slashable_vector_is_proven_with_the_reference_public_values(gpu, keys, name):
    from dvt_circuits_amd import capi

    pk, vk = keys
    scenario, buf = vector(name)
    ec_want, pv_want = dkg_verify.verify_share(scenario)
    assert ec_want == 0 and len(pv_want) == 290
    proof, rep = gpu.prove_core(pk, [buf])
    ok, ec, pv, why = capi.verify(vk, proof)
    assert ok and ec == 0 and rep["exit_code"] == 0, why
    assert pv == pv_want
    assert gpu.prove_core(pk, [buf])[0] == proof
    # a tampered word of the container header, the public values or a shard proof is rejected
    words = np.frombuffer(proof, dtype=np.uint32).copy()
    body = len(words) - sum(1 + len(s) // 4 for s in capi.split_container(proof)[2])   # the first shard's length word
    for pos in (1, 5, body + 1, (body + len(words)) // 2, len(words) - 1):
        w = words.copy()
        w[pos] = (int(w[pos]) + 1) % BABYBEAR
        assert not capi.verify(vk, w.tobytes())[0], f"tampered word {pos} accepted"


def test_a_valid_share_is_not_proven(gpu, keys):
    """the reference panics on a valid share (main.rs:81): the guest halts with exit code 1, so there is no proof"""
    from dvt_circuits_amd import capi

    scenario, buf = vector("seeds-commitment-from-2-to-1.json")
    assert dkg_verify.verify_share(scenario)[0] == 1
    with pytest.raises(capi.DvtError) as e:
        gpu.prove_core(keys[0], [buf])
    assert e.value.code == capi.DVT_ERR_GUEST


def oracle_prove_execution(elf, stdin, log_shard, q, pow_bits):
    """the oracle side end to end, as tests/test_gpu_proof_parity.py builds it: the traces come from the oracle's own guest
    machine + row expansion (oracle/rv32_model.py), not from the product's executor"""
    from oracle import rv32_model

    run = rv32_model.Run(elf, stdin, log_shard)
    assert run.halted and not run.error
    shards = [rv32_model.traces(run, i) for i in range(len(run.shards))]
    prep_root = _oracle_prover.prep_root_of(shards[0][0])
    headers = [_oracle_prover.main_root(chips) + [int(x) for x in pubs] for chips, pubs in shards]
    gc = _oracle_prover.global_challenges(prep_root, headers)
    return [_oracle_prover.prove_shard("rv32", chips, pubs, q, pow_bits, perm_challenges=gc)[0] for chips, pubs in shards]


def test_proof_bytes_equal_oracle_across_shards():
    """the slashable bad-secret-key vector (about 83 k cycles, subgroup checks included) in 2^16-row shards, with few FRI
    queries and little grinding to keep the oracle short: every shard proof equals the oracle CPU prover's"""
    from dvt_circuits_amd import capi

    q, pow_bits, log_shard = 6, 5, 16
    scenario, buf = vector("seeds-commitment-from-2-to-1-bad-secret-key.json")
    elf = gs.bad_share()
    p = capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d}' % (q, pow_bits, log_shard))
    pk, vk = p.setup(elf)
    proof, rep = p.prove_core(pk, [buf])
    ec, pv, gpu_shards = capi.split_container(proof)
    assert ec == 0 and pv == dkg_verify.verify_share(scenario)[1]
    cpu_shards = oracle_prove_execution(elf, [buf], log_shard, q, pow_bits)
    assert len(gpu_shards) == len(cpu_shards) >= 2
    for i, (g, c) in enumerate(zip(gpu_shards, cpu_shards)):
        assert g == c, f"shard {i} differs from the oracle's"
    assert capi.verify(vk, proof, q, pow_bits)[0]
    p.pk_free(pk)
    p.close()


def test_cli_prove_then_verify(tmp_path):
    """`dvt_prover_host prove --type bad-share` with the guest from $DVT_ELF_DIR (tools/build_guests.py), then `verify`"""
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "build_guests.py"), str(tmp_path)], stdout=subprocess.DEVNULL)
    env = dict(os.environ, DVT_ELF_DIR=str(tmp_path))
    inp = tmp_path / "in.json"
    scenario = json.load(open(os.path.join(VECTORS, "seeds-commitment-from-2-to-1-bad-secret-key.json")))["scenario"]
    inp.write_text(json.dumps(scenario))
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "spec_json"), os.path.join(str(tmp_path), "spec", "json"))
    r = subprocess.run([CLI, "prove", "--type", "bad-share", "-i", str(inp), "--json-schema-file", "spec/json/share_exchange_spec.json"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    proof_path = str(inp) + "_proof.bin"
    assert f"Proof saved to: {proof_path}" in r.stdout and os.path.getsize(proof_path) > 1000
    r = subprocess.run([CLI, "verify", "--type", "bad-share", "-i", proof_path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Proof verified" in r.stdout, r.stderr
