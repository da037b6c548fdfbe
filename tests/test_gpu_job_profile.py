"""GPU tests of the execution report of a prepared job (profile_records_kernel through dvt_rv32_job_profile /
Prover.job_profile, and `dvt_prover_host check --show-report`).

The yardstick is the independent model (tests/_profile_ref.py over oracle/rv32_model.py); the host path
(capi.execute_profile) must say the same.  Shapes: bignum(40) at 2^14 cycles per shard is seven shards, four workgroups in
each full one, a ragged last shard of 4160 records and a hottest instruction at 5760; muldiv() at 2^12 retires 4965 distinct
instructions, more than the workgroup's cache has slots; the jump-table guest at 2^10 has shards smaller than one
workgroup's span, and its 129 indirect edges overflow an edge table of 16 slots."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import _profile_ref as ref
from tests import guests, guests_profile
from tests.test_profile_host import blocks_of, entry_of, halt_pc_of

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")
PROGRAM_CHIP, PROGRAM_MULT, PROGRAM_P_PC = 0, 0, 0   # csrc/gen/rv32_cols.h


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


def _job_profile(elf, log_shard, extra="", first=0, stride=1, log_edge_slots=0):
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, [], first=first, stride=stride)
    prof = p.job_profile(pk, job, log_edge_slots)
    n = p.job_shards(job)
    p.job_free(job)
    p.pk_free(pk)
    p.close()
    return prof, n


def _same(a, b):
    """two reports say the same (everything but the time)"""
    sa, sb = dict(a["summary"], ms=0), dict(b["summary"], ms=0)
    assert sa == sb, (sa, sb)
    assert np.array_equal(a["pc_count"], b["pc_count"]) and a["edges"] == b["edges"]
    assert a["syscalls"] == b["syscalls"] and a["opcodes"] == b["opcodes"]


@pytest.mark.parametrize("name, log_shard, shards", [("bignum", 14, 7), ("muldiv", 12, None), ("jump_table", 10, 7)])
def test_job_profile_is_the_models_and_the_hosts(name, log_shard, shards):
    from dvt_circuits_amd import capi

    elf = {"bignum": lambda: guests.bignum(40)[0], "muldiv": lambda: guests.muldiv()[0], "jump_table": guests_profile.jump_table}[name]()
    prof, n = _job_profile(elf, log_shard)
    s = prof["summary"]
    print(name, s)
    run = ref.model_run(elf, (), log_shard)
    assert n == len(run.shards) == s["shards_total"] == s["shards_tallied"] and (shards is None or n == shards)
    ref.same_tables(prof, ref.tally(run), name)
    rc, rep, host, err = capi.execute_profile(elf)
    assert rc == 0 and rep["cycles"] == s["cycles"], err
    ref.same_tables(host, ref.tally(run), name + " on the host")
    assert np.array_equal(prof["pc_count"], host["pc_count"]) and prof["edges"] == host["edges"]
    ref.flow_law(prof, entry_of(elf), halt_pc_of(run))
    if name == "bignum":
        assert s["cycles"] == 102464 and len(run.shards[-1]["rows"]) == 4160 and int(prof["pc_count"].max()) == 5760
    if name == "muldiv":
        assert int((prof["pc_count"] > 0).sum()) > 4096      # more distinct keys than the workgroup's cache has slots


def test_shard_size_does_not_change_the_profile():
    elf = guests.arith(commit=True)[0]
    small, n_small = _job_profile(elf, 10)
    large, n_large = _job_profile(elf, 14)
    assert n_small > 1 and n_large == 1
    for k in ("shards_tallied", "shards_total"):
        small["summary"][k] = large["summary"][k] = 0
    _same(small, large)
    ref.same_tables(small, ref.tally(ref.model_run(elf)), "arith")


def test_pc_count_is_k0s_program_multiplicity():
    """shard by shard: the count of every provable instruction equals the multiplicity K0 wrote into the program chip's table
    of that shard (rows mapped through the preprocessed pc column)"""
    from dvt_circuits_amd import capi

    elf = guests.arith(commit=True)[0]
    host_chips, _, n_total = capi.rv32_debug_traces(elf, (), 10, 0)
    prep_pc = next(c for c in host_chips if c["chip_id"] == PROGRAM_CHIP)["prep"][PROGRAM_P_PC]
    run = ref.model_run(elf, (), 10)
    assert n_total == len(run.shards) > 1
    provable = sorted(i.pc for i in run.provable)
    assert [int(x) for x in prep_pc[:len(provable)]] == provable
    p = _prover(10)
    pk, _ = p.setup(elf)
    for k in range(n_total):
        job, _ = p.prepare(pk, [], first=k, stride=n_total)
        prof = p.job_profile(pk, job)
        chips, _ = p.debug_device_traces(pk, job, k)
        mult = next(c for c in chips if c["chip_id"] == PROGRAM_CHIP)["main"][PROGRAM_MULT]
        tb = prof["summary"]["text_base"]
        got = [int(prof["pc_count"][(pc - tb) // 4]) for pc in provable]
        assert got == [int(x) for x in mult[:len(provable)]], k
        assert int(mult[len(provable):].sum()) == 0 and sum(got) == prof["summary"]["cycles"] == len(run.shards[k]["rows"])
        assert prof["summary"]["shards_tallied"] == 1 and prof["summary"]["shards_total"] == n_total
        p.job_free(job)
    p.pk_free(pk)
    p.close()


def test_a_partial_job_tallies_its_own_shards():
    elf = guests.bignum(40)[0]
    run = ref.model_run(elf, (), 14)
    odd, n = _job_profile(elf, 14, first=1, stride=2)
    assert n == 7 and odd["summary"]["shards_tallied"] == 3 and odd["summary"]["shards_total"] == 7
    want = ref.tally(run, [1, 3, 5])
    ref.same_tables(odd, want, "shards 1, 3, 5")
    # every held shard ends in a record whose successor is the shard's next_pc: three boundary records, each counted once
    assert odd["summary"]["cycles"] == 3 << 14
    even, _ = _job_profile(elf, 14, first=0, stride=2)
    ref.same_tables(even, ref.tally(run, [0, 2, 4, 6]), "shards 0, 2, 4, 6")
    whole, _ = _job_profile(elf, 14)
    assert np.array_equal(odd["pc_count"] + even["pc_count"], whole["pc_count"])
    both = {}
    for a, b, c in odd["edges"] + even["edges"]:
        both[(a, b)] = both.get((a, b), 0) + c
    assert both == {(a, b): c for a, b, c in whole["edges"]}
    assert {k: odd["syscalls"].get(k, 0) + even["syscalls"].get(k, 0) for k in whole["syscalls"]} == whole["syscalls"]
    assert odd["summary"]["n_transfers"] + even["summary"]["n_transfers"] == whole["summary"]["n_transfers"]


def test_a_small_edge_table_drops_and_says_so():
    elf = guests_profile.jump_table()
    want = ref.tally(ref.model_run(elf, (), 10))
    small, _ = _job_profile(elf, 10, log_edge_slots=4)
    s = small["summary"]
    print("16 slots:", s)
    assert s["dropped_transfers"] > 0 and s["n_transfers"] == 704
    assert sum(c for _, _, c in small["edges"]) + s["dropped_transfers"] == s["n_transfers"]
    assert 0 < len(small["edges"]) == s["n_edges"] < 137 and small["edges"] == sorted(small["edges"])
    assert all(want["edges"][(a, b)] == c for a, b, c in small["edges"])
    assert np.array_equal(small["pc_count"], want["pc_count"]) and small["syscalls"] == want["syscalls"] and small["opcodes"] == want["opcodes"]
    full, _ = _job_profile(elf, 10)
    assert full["summary"]["n_edges"] == 137 and full["summary"]["dropped_transfers"] == 0
    ref.same_tables(full, want, "default table")


def _prove_with_and_without_profile(extra):
    """(proof of a job that was profiled before and after, proof of a job that never was); both profiles are equal"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    proofs = []
    for profile in (True, False):
        p = _prover(11, extra)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = p.job_profile(pk, job) if profile else None
        proofs.append(p.prove_job(pk, job))
        if profile:
            _same(before, p.job_profile(pk, job))
            assert p.prove_job(pk, job) == proofs[0]
            ref.same_tables(before, ref.tally(ref.model_run(elf, (), 11)), "commit_only")
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why
    return proofs


@pytest.mark.parametrize("extra", ["", ', "keep_phase1": 0'])
def test_the_job_is_left_as_found(extra):
    with_profile, without = _prove_with_and_without_profile(extra)
    assert with_profile == without


def test_a_profile_drains_a_running_pipeline():
    """two lanes, prove_shard of shard 0 starts the phase-2 pipeline, the profile stops it; the shards proven afterwards
    assemble into the proof of a handle that never profiled"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    containers = []
    for profile in (True, False):
        p = _prover(11, ', "lanes": 2')
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        n = p.job_shards(job)
        assert n == 3
        headers = [p.commit_shard(pk, job, i) for i in range(n)]
        ch = capi.rv32_challenges(vk, headers)
        proofs = [p.prove_shard(pk, job, 0, ch)]
        if profile:
            ref.same_tables(p.job_profile(pk, job), ref.tally(ref.model_run(elf, (), 11)), "after prove_shard(0)")
        proofs += [p.prove_shard(pk, job, i, ch) for i in range(1, n)]
        containers.append(p.assemble(job, proofs))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert containers[0] == containers[1]
    ok, ec, pv, why = capi.verify(vk, containers[0], Q, POW)
    assert ok and pv == b"check me", why


def test_two_members_give_the_one_device_profile():
    elf = guests.bignum(40)[0]
    one, _ = _job_profile(elf, 14)
    two, n = _job_profile(elf, 14, ', "devices": [0, 0]')
    assert n == 7
    _same(one, two)


def test_cli_check_show_report(tmp_path):
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    want = ref.tally(ref.model_run(elf))
    r = subprocess.run([CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path), "--show-report"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ") and " shards, " in r.stdout and " chip tables, " in r.stdout
    assert r.stdout.splitlines()[1].startswith("opcode counts (")
    n_ops, ops, n_sys, sysc = blocks_of(r.stdout)
    assert n_ops == want["cycles"] and ops == want["opcodes"]
    assert n_sys == sum(want["syscalls"].values()) and sysc == {"halt": 1, "write": 1, "commit": 8}
    plain = subprocess.run([CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path)], capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith("clean: ") and len(plain.stdout.splitlines()) == 1
