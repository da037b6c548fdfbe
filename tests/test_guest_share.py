"""CPU tests: the reference's bad-share guest re-stated for this machine (tests/guests_share.py; reference
crates/bad_share_exchange_prove/src/main.rs + crates/dkg/src/verification.rs:91-183) on the reference's OWN inputs.

* the reference's 10 no-auth share vectors (test_vectors/no_auth/share/*.json, copied as data fixtures to
  tests/golden/share_vectors/): `execute` ends with every vector's expected exit code, a slashable run commits exactly the
  bytes of the Python restatement (tools/dkg_verify.verify_share), which agrees with the vectors too;
* synthetic inputs built with tools/bls12_381.py reach the branches no vector reaches alone: a correct share, a secret equal
  to r, a base pubkey off the curve, inputs beyond the guest's tables, the empty polynomial, the ids 1 and n;
* the reference's harness shape through the host CLI; the run satisfies the AIR shard by shard."""
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys

import pytest

from dvt_circuits_amd import capi
from tests import _orc, guests_share as gs
from tests.test_rv32_exec_trace import check_traces
from tools import bls12_381 as B
from tools import dkg_verify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = os.path.join(ROOT, "tests", "golden", "share_vectors")


@pytest.fixture(scope="module")
def elf():
    return gs.bad_share(nmax=8, kmax=8)


def run(elf, scenario):
    """-> (exit code, public values) of the guest on the scenario through the host encoder"""
    buf = capi.stdin_from_json("bad-share", json.dumps(scenario).encode())
    rc, rep, pv, out, err = capi.execute_io(elf, [buf])
    assert rc in (0, capi.DVT_ERR_GUEST) and rep["halted"] and not rep["unprovable"], err
    assert rep["exit_code"] == (0 if rc == 0 else 1)
    return rep["exit_code"], pv


def test_reference_vectors_end_with_their_expected_exit_codes(elf):
    files = sorted(glob.glob(os.path.join(VECTORS, "*.json")))
    assert len(files) == 10
    seen = {0: 0, 1: 0}
    for path in files:
        vec = json.load(open(path))
        want = int(vec["params"]["expected_exit_code"])
        name = os.path.basename(path)
        ec, pv = run(elf, vec["scenario"])
        assert ec == want, (name, want, ec)
        py_ec, py_pv = dkg_verify.verify_share(vec["scenario"])
        assert py_ec == want, (name, want, py_ec)
        seen[want] += 1
        if want == 0:
            n = vec["scenario"]["initial_commitment"]["settings"]["n"]
            assert pv == py_pv and len(pv) == n * (8 + 64) + (8 + 66), name    # 290 bytes at n = 3
        else:
            assert pv == b""
    assert seen == {0: 3, 1: 7}


# ------------------------------------------------------------------------------------------------ synthetic inputs
def _h(tag, i):
    return hashlib.sha256(b"%s %d" % (tag, i)).digest()


def scenario(n=3, k=2, own=1, dst=0, sk=None, pubkeys=None):
    """n base hashes, the `own`-th of which is the initial commitment of a degree k - 1 polynomial; the share is sent to
    base hash number `dst` (input order); sk = the correct share for that destination unless given"""
    cfs = [int.from_bytes(_h(b"coefficient", i), "big") % B.R for i in range(k)]
    pks = pubkeys if pubkeys is not None else [B.g1_compress(B.E1.mul(B.G1, c)) for c in cfs]
    gen_id = _h(b"gen_id", 0)[:16]
    ic = dkg_verify.commitment_hash(gen_id, n, k, pks)
    hashes = [_h(b"base hash", i) for i in range(n)]
    hashes[own] = ic
    dest = hashes[dst]
    dest_id = sorted(hashes).index(dest) + 1
    if sk is None:
        sk = sum(c * pow(dest_id, i, B.R) for i, c in enumerate(cfs)) % B.R
    return {
        "base_hashes": [h.hex() for h in hashes],
        "initial_commitment": {"hash": ic.hex(), "settings": {"gen_id": gen_id.hex(), "n": n, "k": k},
                               "base_pubkeys": [p.hex() for p in pks]},
        "seeds_exchange_commitment": {
            "initial_commitment_hash": ic.hex(),
            "ssecret": {"shared_secret": sk.to_bytes(32, "big").hex(), "dst_base_hash": dest.hex()},
            "commitment": {"hash": _h(b"commitment", 0).hex(), "pubkey": "02" + _h(b"secp", 0).hex(),
                           "signature": (_h(b"sig", 0) + _h(b"sig", 1)).hex()},
        },
    }


def check(elf, sc, want):
    """the guest and the Python restatement agree with each other and with the expected exit code"""
    py_ec, py_pv = dkg_verify.verify_share(sc)
    assert py_ec == want
    ec, pv = run(elf, sc)
    assert ec == want and pv == py_pv
    if want == 0:
        assert len(pv) == len(sc["base_hashes"]) * 72 + 74


def test_a_correct_share_is_not_slashable(elf):
    check(elf, scenario(), 1)
    check(elf, scenario(n=5, k=4, own=3, dst=2), 1)


def test_a_secret_equal_to_r_is_slashable(elf):
    check(elf, scenario(sk=B.R), 0)
    check(elf, scenario(sk=(1 << 256) - 1), 0)


def test_a_wrong_share_is_slashable(elf):
    good = int(scenario()["seeds_exchange_commitment"]["ssecret"]["shared_secret"], 16)
    check(elf, scenario(sk=(good + 1) % B.R), 0)


def test_a_base_pubkey_off_the_curve_panics(elf):
    x = next(x for x in range(1, 100) if B.fp_sqrt((x ** 3 + 4) % B.P) is None)
    off = bytearray(x.to_bytes(48, "big"))
    off[0] |= 0x80
    good = scenario()["initial_commitment"]["base_pubkeys"]
    check(elf, scenario(pubkeys=[bytes.fromhex(good[0]), bytes(off)]), 1)
    # a non-canonical encoding of the point at infinity is rejected as well (G1Affine::from_compressed)
    check(elf, scenario(pubkeys=[bytes.fromhex(good[0]), bytes([0xC0]) + bytes(46) + b"\x01"]), 1)


def test_no_coefficients_evaluate_to_the_identity(elf):
    check(elf, scenario(k=0, sk=0), 1)
    check(elf, scenario(k=0, sk=1), 0)


def test_inputs_beyond_the_tables_exit_1():
    """slashable inputs, which the guest refuses only because they exceed its nmax / kmax tables"""
    small = gs.bad_share(nmax=4, kmax=2)
    for sc in (scenario(n=5, k=2, sk=B.R), scenario(n=3, k=3, sk=B.R)):
        assert dkg_verify.verify_share(sc)[0] == 0
        assert run(small, sc) == (1, b"")
    check(small, scenario(n=4, k=2, sk=B.R), 0)


def test_destination_ids_1_and_n(elf):
    """the destination's id is its rank among the byte-wise sorted base hashes + 1 (verification.rs:50-66, :125-126):
    the share of the first and of the last hash is accepted, the share of a neighbouring id is slashable"""
    n = 4
    hashes = bytes.fromhex("".join(scenario(n=n, k=3, own=1)["base_hashes"]))
    order = sorted(range(n), key=lambda i: hashes[32 * i:32 * i + 32])
    first, last = order[0], order[-1]
    for dst, dest_id, other_id in ((first, 1, 2), (last, n, n - 1)):
        sc = scenario(n=n, k=3, own=1, dst=dst)
        check(elf, sc, 1)
        wrong = scenario(n=n, k=3, own=1, dst=order[other_id - 1])["seeds_exchange_commitment"]["ssecret"]["shared_secret"]
        check(elf, scenario(n=n, k=3, own=1, dst=dst, sk=int(wrong, 16)), 0)


def test_cli_harness_on_the_vectors(tmp_path):
    """the reference's harness shape (tools/run_vectors.py = script/run.sh) through the host CLI with the guest from $DVT_ELF_DIR"""
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "build_guests.py"), str(tmp_path)], stdout=subprocess.DEVNULL)
    assert (tmp_path / "bad-share.elf").exists()
    env = dict(os.environ, DVT_ELF_DIR=str(tmp_path))
    # (the vectors name their schema relative to the reference's root: spec/json/share_exchange_spec.json)
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "spec_json"), os.path.join(str(tmp_path), "spec", "json"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_vectors.py"), "--cwd", str(tmp_path), VECTORS],
                       capture_output=True, text=True, env=env, timeout=600)
    assert "passed 10  failed 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.returncode == 0


def test_the_run_satisfies_the_air():
    """a slashable vector without the subgroup checks and cut into small shards keeps the Python-side multiset check short;
    the run still exercises the cpu, bls_g1 (decompression, Horner, [sk] G) and mem_init chips"""
    air = _orc.air("rv32")
    vec = json.load(open(os.path.join(VECTORS, "seeds-commitment-from-2-to-1-bad-secret-key.json")))
    buf = capi.stdin_from_json("bad-share", json.dumps(vec["scenario"]).encode())
    small = gs.bad_share(nmax=4, kmax=4, subgroup_check=False)
    rc, rep, pv, out, err = capi.execute_io(small, [buf])
    assert rc == 0 and pv == dkg_verify.verify_share(vec["scenario"])[1]
    log_shard = 15
    check_traces(air, small, [buf], log_shard=log_shard)
    names, shard, n_shards = set(), 0, 1
    while shard < n_shards:
        chips, pubs, n_shards = capi.rv32_debug_traces(small, [buf], log_shard, shard)
        names |= {air.chip(c["chip_id"]).name.decode() for c in chips}
        shard += 1
    assert n_shards >= 2 and {"cpu", "bls_g1", "mem_init"} <= names, names
