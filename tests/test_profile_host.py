"""The execution report on the host (dvt_execute_profile, no GPU) against the independent model (tests/_profile_ref.py): the
four tables of seven guests, the flow law from the report's own outputs, an instruction without a chip, a failing guest, the
CLI's two count blocks, and the finalization guest on the reference's example."""
import json
import os
import re
import struct
import subprocess

import pytest

from dvt_circuits_amd import capi
from tests import _profile_ref as ref
from tests import guests, guests_profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")
GOLD = os.path.join(ROOT, "tests", "golden")
SYS_SHA_EXTEND, SYS_SHA_COMPRESS = 0x00300105, 0x00010106
CURVE_IDS = (0x0001010A, 0x0000010B, 0x0001011E, 0x0000011F)   # secp256k1 add / double, bls12381 add / double
G1_IDS, FP_IDS, U256_ID = (0x0001011E, 0x0000011F), (0x00010120, 0x00010121, 0x00010122), 0x0001011D

GUESTS = {
    "arith": lambda: guests.arith(commit=True)[0],
    "shifts": lambda: guests.shifts()[0],
    "muldiv": lambda: guests.muldiv()[0],
    "subword": lambda: guests.subword()[0],
    "sha256_precompiled": lambda: guests.sha256_precompiled(bytes(range(70)))[0],
    "curve_ops": lambda: guests.curve_ops()[0],
    "jump_table": guests_profile.jump_table,
}


def entry_of(elf):
    return struct.unpack_from("<I", elf, 24)[0]


def halt_pc_of(run):
    return run.shards[-1]["rows"][-1].ins.pc


@pytest.mark.parametrize("name", sorted(GUESTS))
def test_host_report_is_the_models(name):
    elf = GUESTS[name]()
    rc, rep, prof, err = capi.execute_profile(elf)
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    run = ref.model_run(elf)
    want = ref.tally(run)
    ref.same_tables(prof, want, name)
    s = prof["summary"]
    assert s["cycles"] == rep["cycles"] == run.cycles and s["dropped_transfers"] == 0
    assert s["n_instr"] == run.n_instr and s["text_base"] == run.text_base and s["shards_tallied"] == s["shards_total"] == 1
    ref.flow_law(prof, entry_of(elf), halt_pc_of(run))
    if name == "sha256_precompiled":
        assert prof["syscalls"][SYS_SHA_EXTEND] == want["syscalls"][SYS_SHA_EXTEND] > 0
        assert prof["syscalls"][SYS_SHA_COMPRESS] == want["syscalls"][SYS_SHA_COMPRESS] > 0
    if name == "curve_ops":
        assert all(prof["syscalls"][i] == want["syscalls"][i] > 0 for i in CURVE_IDS)
    if name == "jump_table":
        jalr = [e for e in prof["edges"] if ref.mnemonic(run.text[e[0]].word) == "jalr"]
        assert (s["cycles"], s["n_edges"], len(jalr), s["n_transfers"]) == (6396, 137, 129, 704)
    if name == "arith":
        assert (s["n_edges"], s["n_transfers"]) == (58, 307)


def test_an_instruction_without_a_chip_is_counted():
    elf = guests.uses_unprovable()
    rc, rep, prof, err = capi.execute_profile(elf)
    assert rc == 0 and rep["unprovable"] and rep["halted"], err
    assert prof["opcodes"].get("fence") == 1 and prof["summary"]["cycles"] == rep["cycles"] == capi.execute(elf)[1]["cycles"]
    assert int(prof["pc_count"].sum()) == rep["cycles"] and prof["syscalls"] == {0: 1}
    ref.flow_law(prof, entry_of(elf), prof["summary"]["text_base"] + 4 * (prof["summary"]["n_instr"] - 1))


def test_a_failing_guest_answers_as_execute_does():
    elf = guests.exit_with(1)
    rc, rep, prof, err = capi.execute_profile(elf)
    rc0, rep0, _, err0 = capi.execute(elf)
    assert rc == rc0 == capi.DVT_ERR_GUEST and rep == rep0 and err == err0
    assert prof["summary"]["cycles"] == rep["cycles"]          # the report of what retired comes back all the same


def blocks_of(stdout):
    """the two count blocks of --show-report: (N of the opcode line, {name: count}, N of the syscall line, {name: count})"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("opcode counts ("))
    b = next(i for i, l in enumerate(lines) if l.startswith("syscall counts ("))
    n_ops = int(re.fullmatch(r"opcode counts \((\d+) total instructions\):", lines[a]).group(1))
    n_sys = int(re.fullmatch(r"syscall counts \((\d+) total syscall instructions\):", lines[b]).group(1))
    ops = [(l.split()[1], int(l.split()[0])) for l in lines[a + 1:b]]
    sysc = [(l.split()[1], int(l.split()[0])) for l in lines[b + 1:]]
    for rows in (ops, sysc):   # by count descending, then by name
        assert rows == sorted(rows, key=lambda r: (-r[1], r[0]))
    return n_ops, dict(ops), n_sys, dict(sysc)


def test_cli_execute_show_report(tmp_path):
    path = tmp_path / "hint_sum.elf"
    path.write_bytes(guests.hint_sum())
    inp = os.path.join(GOLD, "finalization_example.json")
    r = subprocess.run([CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path), "--show-report"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    rc, rep, prof, err = capi.execute_profile(guests.hint_sum(), [buf])
    head = f"input len: {len(buf) - 8}\nVerification report:\ntotal instructions: {rep['cycles']}\nexit code: 0\nopcode counts ("
    assert r.stdout.startswith(head), r.stdout[:300]
    n_ops, ops, n_sys, sysc = blocks_of(r.stdout)
    assert n_ops == rep["cycles"] and ops == prof["opcodes"] and sum(ops.values()) == n_ops
    assert n_sys == sum(prof["syscalls"].values()) and sysc == {"halt": 1, "write": 1, "commit": 8, "hint_len": 1, "hint_read": 1}
    # without the flag nothing of it is printed
    r = subprocess.run([CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == f"input len: {len(buf) - 8}\n"


def test_finalization_guest_on_the_reference_example():
    from tests import guests_finalization as gf

    example = open(os.path.join(GOLD, "finalization_example.json"), "rb").read()
    buf = capi.stdin_from_json("finalization", example)
    elf = gf.finalization(nmax=8, kmax=8)
    rc, rep, prof, err = capi.execute_profile(elf, [buf])
    rc0, rep0, pv, _ = capi.execute(elf, [buf])
    assert rc == rc0 == 0 and rep == rep0 and pv == gf.expected_public_values(json.loads(example)), err
    assert prof["summary"]["cycles"] == rep0["cycles"] and prof["summary"]["dropped_transfers"] == 0
    run = ref.model_run(elf, [buf])
    ref.flow_law(prof, entry_of(elf), halt_pc_of(run))
    want = ref.tally(run)
    family = lambda table, ids: sum(table.get(i, 0) for i in ids)
    for ids in (G1_IDS, FP_IDS, (U256_ID,)):
        assert family(prof["syscalls"], ids) == family(want["syscalls"], ids) > 0
    print("G1 %d, Fp %d, UINT256_MUL %d calls" % tuple(family(prof["syscalls"], ids) for ids in (G1_IDS, FP_IDS, (U256_ID,))))
    ref.same_tables(prof, want, "finalization")
