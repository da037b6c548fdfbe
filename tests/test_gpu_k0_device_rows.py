"""K0 of the muldiv, sha_extend and sha_compress chips on the GPU: the product path uploads the events of these chips and the
device expands them into trace rows (k0_aux_rows_kernel), as it does for the shift chip.  The device-built traces of every
chip of every shard (the byte chip included: a miscounted lookup shows there) must equal, cell by cell, (a) the oracle's
independent Python statement of the machine and of the rows (oracle/rv32_model.py) and (b) the product's host-side
expansion, which runs the same row templates on the CPU; and the job must report that these chips' rows were built on the
device (job_shard_device_rows)."""
import numpy as np
import pytest

from tests import guests
from tools.rvasm import Asm

pytestmark = pytest.mark.gpu

CFG = '"fri_queries": 8, "pow_bits": 4'
MULDIV, SHA_EXTEND, SHA_COMPRESS = 6, 7, 8   # chip ids (tools/airgen/rv32.py)


def muldiv_loop(iters=700):
    """6 * iters + 8 instructions of the muldiv chip: RISC-V's special cases first (division by zero in all four forms,
    INT_MIN / -1 in both, MULH of two negatives, MULHSU with a negative first operand), then a loop that applies all six
    operations to a pair of operands stepped by a multiplicative recurrence (both signs, all magnitudes)"""
    a = Asm()
    out = a.dword("out", [0] * 4)
    a.li("s10", 0)

    def fold(op, b, c):
        a.li("a3", b)
        a.li("a4", c)
        getattr(a, op)("a5", "a3", "a4")
        a.xor("s10", "s10", "a5")

    for op in ("div", "divu", "rem", "remu"):
        fold(op, 0x12345678, 0)
    fold("div", 0x80000000, 0xFFFFFFFF)
    fold("rem", 0x80000000, 0xFFFFFFFF)
    fold("mulh", 0xFFFF8001, 0x80000003)
    fold("mulhsu", 0xDEADBEEF, 0xFFFFFFF1)
    a.li("a3", 0x9E3779B9)
    a.li("a4", 0x7F4A7C15)
    a.li("s5", 1664525)
    a.li("s6", 1013904223)
    a.li("s7", 0x85EBCA6B)
    a.li("s4", iters)
    a.label("again")
    a.mul("a3", "a3", "s5")
    a.add("a3", "a3", "s6")
    a.add("a4", "a4", "a3")
    a.xor("a4", "a4", "s7")
    for op in ("mulh", "mulhsu", "div", "divu", "rem", "remu"):
        getattr(a, op)("a5", "a3", "a4")
        a.xor("s10", "s10", "a5")
    a.addi("s4", "s4", -1)
    a.bne("s4", "zero", "again")
    a.li("s0", out)
    a.sw("s10", "s0", 0)
    guests._finish(a, out, 4)
    return a.elf()


def _compare(want, got, shard, what):
    assert len(want) == len(got)
    for w, d in zip(want, got):
        assert w["chip_id"] == d["chip_id"] and w["log_n"] == d["log_n"]
        diff = np.argwhere(w["main"] != d["main"])
        detail = [(int(c), int(r), int(w["main"][c, r]), int(d["main"][c, r])) for c, r in diff[:12]]
        assert diff.size == 0, f"shard {shard} chip {w['chip_id']}: {len(diff)} cells differ from {what}, first (col,row,{what},dev): {detail}"


def _check_parity(elf, log_shard, min_log_n=None):
    """every shard: device traces == model == host expansion; the device_rows mask names chips 6, 7, 8 exactly where they
    are present.  Returns {chip id: shards in which it is present}."""
    from dvt_circuits_amd import capi
    from oracle import rv32_model

    p = capi.Prover('{%s, "log_shard_size": %d}' % (CFG, log_shard))
    pk, _ = p.setup(elf)
    job, rep = p.prepare(pk, [])
    n = p.job_shards(job)
    run = rv32_model.Run(elf, [], log_shard)
    assert n == len(run.shards) and rep["cycles"] == run.cycles
    seen = {MULDIV: 0, SHA_EXTEND: 0, SHA_COMPRESS: 0}
    for shard in range(n):
        dev, dpubs = p.debug_device_traces(pk, job, shard)
        model, mpubs = rv32_model.traces(run, shard)
        host, hpubs, _ = capi.rv32_debug_traces(elf, [], log_shard, shard)
        assert (dpubs == mpubs).all() and (dpubs == hpubs).all()
        _compare(model, dev, shard, "model")
        _compare(host, dev, shard, "host")
        present = {d["chip_id"]: d["log_n"] for d in dev}
        mask = p.job_shard_device_rows(job, shard)
        for c in seen:
            assert bool(mask >> c & 1) == (c in present), f"shard {shard}: device_rows {mask:#x}, chip {c} present: {c in present}"
            seen[c] += c in present
            if min_log_n and c in min_log_n and c in present:
                assert present[c] == min_log_n[c], f"chip {c}: 2^{present[c]} rows"
    assert p.job_shard_device_rows(job, n) == 0      # (no such shard)
    p.job_free(job)
    p.pk_free(pk)
    p.close()
    return seen


@pytest.mark.parametrize("which,log_shard", [("muldiv", 9), ("sha_extend", 10), ("sha256", 21), ("sha256", 10)])
def test_device_rows_equal_model_and_host_rows(which, log_shard):
    """(sha256 at 2^10: a run of several shards, whose SHA rows read words last accessed under another shard number,
    m_same = 0)"""
    elf = {"muldiv": lambda: guests.muldiv()[0], "sha_extend": lambda: guests.sha_extend(3)[0],
           "sha256": lambda: guests.sha256_precompiled(bytes(range(150)))[0]}[which]()
    seen = _check_parity(elf, log_shard)
    if which == "muldiv":
        assert seen[MULDIV] >= 2 and not seen[SHA_EXTEND] and not seen[SHA_COMPRESS]
    elif which == "sha_extend":
        assert seen[SHA_EXTEND] and not seen[SHA_COMPRESS]
    else:
        assert seen[SHA_EXTEND] and seen[SHA_COMPRESS]


def test_sha_rows_past_one_workgroup():
    """65 blocks: 4160 sha_extend rows and 5200 sha_compress rows, both past the 4096 rows of one workgroup, neither a power
    of two (padded to 2^13); a workgroup boundary falls inside a compress call"""
    elf = guests.sha256_precompiled(bytes(i % 251 for i in range(4100)))[0]
    seen = _check_parity(elf, 21, {SHA_EXTEND: 13, SHA_COMPRESS: 13})
    assert seen[SHA_EXTEND] == 1 and seen[SHA_COMPRESS] == 1


def test_muldiv_rows_past_one_workgroup():
    """4208 muldiv rows (padded to 2^13) over varied operands and every special case"""
    seen = _check_parity(muldiv_loop(700), 21, {MULDIV: 13})
    assert seen[MULDIV] == 1


def test_phase2_recompute_proves_the_same_bytes():
    """"keep_phase1": 0 makes phase 2 run K0 again: it must find the device-built rows of these chips, not a host table"""
    from dvt_circuits_amd import capi

    elf, _ = guests.sha256_precompiled(bytes(range(150)))
    proofs = []
    for extra in ('"keep_phase1": 0, ', ""):
        p = capi.Prover('{%s%s, "log_shard_size": 10}' % (extra, CFG))
        pk, vk = p.setup(elf)
        proof, rep = p.prove_core(pk, [])
        ok, ec, _, why = capi.verify(vk, proof, 8, 4)
        assert ok and ec == 0, why
        proofs.append(proof)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
