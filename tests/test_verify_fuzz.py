"""CPU test: the untrusted-input side of the library — dvt_verify's container parser
(csrc/proof.h, csrc/capi_rv32.hip) and the shard verifier (csrc/verifier.hip) — built host-only with AddressSanitizer +
UBSan (`make -C dvt_circuits_amd/csrc asan-fuzz`; sanitizers run on the CPU build only) and driven with byte mutations,
truncations, splices and hostile length words of valid proofs (tools/fuzz/fuzz_verify.cpp).  Every outcome must be a clean
DVT_ERR_REJECTED / DVT_ERR_INPUT; any memory error or undefined behaviour aborts the driver.

The proofs are fixtures made on a GPU box by tools/make_proof_fixture.py (tests/golden/proof_*.bin: a COMMIT-only guest
and the curve-precompile guest, 4 FRI queries): tests/test_gpu_fixtures.py checks on the GPU that they are current."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "build", "asan", "fuzz_verify")
Q, POW = 4, 4


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-j6", "-C", os.path.join(ROOT, "dvt_circuits_amd", "csrc"), "asan-fuzz"],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return FUZZ


@pytest.mark.parametrize("name,iters", [("commit", 4000), ("curve", 1200)])
def test_mutated_proofs_are_rejected_cleanly_under_asan_and_ubsan(driver, name, iters):
    fixture = os.path.join(ROOT, "tests", "golden", f"proof_{name}.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver, fixture, str(iters), "7", str(Q), str(POW)], capture_output=True, text=True, env=env, timeout=900)
    if r.returncode == 3:
        pytest.skip("tests/golden/proof_%s.bin no longer verifies (the AIR or the proof format changed): regenerate it with "
                    "tools/make_proof_fixture.py on a GPU box" % name)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    assert stats["other"] == 0 and stats["iterations"] == iters
    # (only no-op mutations — a length word overwritten with its own value — leave a proof valid; a first run of this test
    #  found one real slack: bytes after the NUL of the machine name in the verifying key were ignored, now rejected)
    assert stats["rejected"] + stats["input"] >= iters * 0.99, stats
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
