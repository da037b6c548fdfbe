"""GPU tests of dvt_rv32_check_job (Prover.check_job) and of `dvt_prover_host check`: honest jobs are clean and balanced, the
check leaves the job as it found it (the proof bytes after a check are those of a handle that never checked), on one
device and on two members of one GPU, and a job that holds only part of the execution is checked without the bus balance."""
import os
import subprocess

import pytest

from tests import guests

pytestmark = pytest.mark.gpu
Q, POW = 8, 4
CFG = '"fri_queries": %d, "pow_bits": %d' % (Q, POW)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _precompile_guest():
    """SHA-256 through the two SHA precompiles and the curve precompiles, in one guest"""
    return guests.dkg_like("finalization", sig_iters=1, pt_iters=1, pair_iters=1, sha_precompiles=True, curve_precompiles=True)


def _clean(summary, findings, bus_checked=1):
    assert summary["ok"] and summary["violations"] == 0 and summary["n_findings"] == 0 and findings == [], summary
    assert summary["bus_checked"] == bus_checked and summary["unbalanced_buses"] == 0, summary
    assert summary["ms"] > 0


def _prove_with_and_without_check(extra):
    from dvt_circuits_amd import capi

    elf, want = guests.commit_only(b"check me"), b"check me"
    proofs = []
    for check in (True, False):
        p = capi.Prover('{%s, "log_shard_size": 11%s}' % (CFG, extra))
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        if check:
            _clean(*p.check_job(pk, job))
        proofs.append(p.prove_job(pk, job))
        if check:   # after the proof the phase-1 results are consumed: the check runs K0 again and is still clean
            _clean(*p.check_job(pk, job))
            assert p.prove_job(pk, job) == proofs[0]
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == want, why
    return proofs


def test_check_job_is_clean_on_honest_jobs():
    from dvt_circuits_amd import capi

    p = capi.Prover('{%s, "log_shard_size": 11}' % CFG)
    pk, _ = p.setup(guests.commit_only(b"check me"))
    job, _ = p.prepare(pk, [])
    assert p.job_shards(job) == 3
    summary, findings = p.check_job(pk, job)
    print("three-shard job:", summary)
    _clean(summary, findings)
    assert all(p.job_shard_chips(job, s) & 0b1111 == 0b1111 for s in range(3)) and p.job_shard_chips(job, 3) == 0
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_check_job_is_clean_on_a_precompile_guest():
    from dvt_circuits_amd import capi

    with open(os.path.join(ROOT, "tests", "golden", "finalization_example.json"), "rb") as f:
        buf = capi.stdin_from_json("finalization", f.read())
    elf = _precompile_guest()
    p = capi.Prover('{%s, "log_shard_size": 12}' % CFG)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, [buf])
    chips = 0
    for s in range(p.job_shards(job)):
        chips |= p.job_shard_chips(job, s)
    assert chips >> 7 & 3 == 3 and chips >> 9, f"the guest must use the SHA and the field / curve precompile chips (mask {chips:#x})"
    summary, findings = p.check_job(pk, job)
    print("precompile guest:", summary)
    _clean(summary, findings)
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_proof_after_check_is_byte_identical():
    with_check, without = _prove_with_and_without_check("")
    assert with_check == without


def test_proof_after_check_is_byte_identical_on_two_members():
    with_check, without = _prove_with_and_without_check(', "devices": [0, 0]')
    assert with_check == without


def test_partial_job_skips_the_bus_balance():
    from dvt_circuits_amd import capi

    p = capi.Prover('{%s, "log_shard_size": 11}' % CFG)
    pk, _ = p.setup(guests.commit_only(b"check me"))
    job, _ = p.prepare(pk, [], first=0, stride=2)
    assert p.job_shards(job) == 3
    summary, findings = p.check_job(pk, job)
    _clean(summary, findings, bus_checked=0)
    p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_host_cli_check_prints_clean(tmp_path):
    from dvt_circuits_amd import capi

    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    with open(example, "rb") as f:
        buf = capi.stdin_from_json("finalization", f.read())
    elf, _ = guests.finalization_like(2, buf, limbs=3)
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    cli = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")
    r = subprocess.run([cli, "check", "--type", "finalization", "-i", example, "--elf", str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ") and " shards, " in r.stdout and " chip tables, " in r.stdout
