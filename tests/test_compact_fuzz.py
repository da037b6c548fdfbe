"""CPU test: the compact proof form on the untrusted-input side of the library (dvt_verify, dvt_proof_compact and
dvt_proof_expand on "DVP2" shards) built host-only with AddressSanitizer + UBSan (`make -C dvt_circuits_amd/csrc
asan-fuzz-compact`; sanitizers run on the CPU build only) and driven by tools/fuzz/fuzz_compact.cpp with mutations,
truncations, splices, flipped magics and hostile count words of the compacted fixtures.  The driver is a plain program:
any memory error or undefined behaviour aborts it, every other outcome must be a clean return code."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "build", "asan", "fuzz_compact")
Q, POW = 4, 4


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-s", "-j6", "-C", os.path.join(ROOT, "dvt_circuits_amd", "csrc"), "asan-fuzz-compact"],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return FUZZ


@pytest.mark.parametrize("name,iters", [("commit", 200), ("curve", 60)])
def test_mutated_compact_proofs_come_back_cleanly_under_asan_and_ubsan(driver, name, iters):
    fixture = os.path.join(ROOT, "tests", "golden", f"proof_{name}.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([driver, fixture, str(iters), "7", str(Q), str(POW)], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    stats = json.loads(r.stdout.strip().splitlines()[-1])
    # three entry points per mutated proof; a mutation that leaves the proof valid (a word overwritten with its own value)
    # is rare, and the transcoders accept what passes the host part, so only the verifier's share is bounded
    assert stats["other"] == 0 and stats["iterations"] == iters
    assert stats["ok"] + stats["rejected"] + stats["input"] == 3 * iters
    assert stats["rejected"] + stats["input"] >= iters * 0.99, stats
    assert "runtime error" not in r.stderr, r.stderr[-3000:]
