"""The divergence entry points of the C ABI (no GPU): they exist, the structs have the sizes of include/dvt_prover.h, the constants
of the Python mirror are the header's, and every input error is refused with DVT_ERR_INPUT."""
import ctypes as C
import os
import re

from dvt_circuits_amd import capi
from tests import guests

ELF = guests.hint_sum()
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvt_prover.h")
A, B = bytes(range(32)), bytes(range(1, 33))


def test_entry_points_sizes_and_version():
    lib = capi.load()
    assert lib.dvt_abi_version() >= 20
    for name in ("dvt_rv32_job_diverge", "dvt_rv32_job_diverge_times", "dvt_execute_diverge"):
        assert hasattr(lib, name), name
    assert (C.sizeof(capi.DivergePos), C.sizeof(capi.DivergeRec), C.sizeof(capi.DivergePair), C.sizeof(capi.DivergeReg), C.sizeof(capi.DivergeSummary)) == \
        (8, 32, 96, 40, 272)
    text = open(HEADER).read()
    for line in ("#define DVT_DIVERGE_SPAN 4096", "#define DVT_DIVERGE_MAX_KEEP 64", "#define DVT_DIVERGE_MAX_WINDOW 16384", "#define DVT_DIVERGE_DEFAULT_WINDOW 4096",
                 "#define DVT_DIV_NONE 0xffffffffffffffffull", "#define DVT_DIVERGE_NO_REJOIN 0xffffffffu",
                 "enum { DVT_DIV_RD = 1, DVT_DIV_RS1 = 2, DVT_DIV_RS2 = 4, DVT_DIV_MEM = 8 };", "enum { DVT_DIVERGE_REJOIN = 1 };",
                 "enum { DVT_DIV_SPLIT = 1, DVT_DIV_BAD = 2, DVT_DIV_END_BOTH = 3, DVT_DIV_END_A = 4, DVT_DIV_END_B = 5, DVT_DIV_LIMIT = 6 };"):
        assert line in text, line
    log = re.search(r"#define DVT_DIVERGE_BATCH_PAIRS \(1u << (\d+)\)", text)
    assert log and capi.DVT_DIVERGE_BATCH_PAIRS == 1 << int(log.group(1))
    for cls, name in ((capi.DivergePos, "dvt_diverge_pos"), (capi.DivergeRec, "dvt_diverge_rec")):
        assert "typedef struct { uint32_t %s; } %s;" % (", ".join(f for f, _ in cls._fields_), name) in text, name
    # the field order of the two larger mirrors is the header's
    for cls, name in ((capi.DivergePair, "dvt_diverge_pair"), (capi.DivergeSummary, "dvt_diverge_summary"), (capi.DivergeReg, "dvt_diverge_reg")):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(uint64_t|uint32_t|float|dvt_diverge_rec)\s", "", decl.strip()).split(",") if f.strip()]
        assert fields == [f for f, _ in cls._fields_], name


def _call(first, last, regs, s, elf=ELF, flags=0, window=0, keep=4, log_shard=0):
    lib = capi.load()
    err = C.c_char_p()
    rc = lib.dvt_execute_diverge(elf, len(elf) if elf else 0, A, len(A), B, len(B), 0, log_shard, capi.DivergePos(1, 0), capi.DivergePos(1, 0), 0, flags, window,
                                 keep, first, last, regs, s, None, None, C.byref(err))
    return rc, capi._take_str(lib, err)


def test_null_arguments_and_limits_are_refused():
    first, last, regs, s = (capi.DivergePair * 64)(), (capi.DivergePair * 64)(), (capi.DivergeReg * 32)(), capi.DivergeSummary()
    rc, err = _call(first, last, regs, C.byref(s))
    assert rc == capi.DVT_OK and s.reason == capi.DVT_DIV_END_BOTH and s.n_data > 0 and s.n_kept == 4, err
    assert _call(first, last, regs, None)[0] == capi.DVT_ERR_INPUT
    assert _call(first, last, regs, C.byref(s), elf=None)[0] == capi.DVT_ERR_INPUT
    for bad in (dict(first=None), dict(last=None), dict(regs=None)):
        args = dict(first=first, last=last, regs=regs)
        args.update(bad)
        rc, err = _call(args["first"], args["last"], args["regs"], C.byref(s))
        assert rc == capi.DVT_ERR_INPUT and "null" in err, bad
    # no pair arrays are needed for no pairs
    assert _call(None, None, regs, C.byref(s), keep=0)[0] == capi.DVT_OK and s.n_kept == 0 and s.n_data > 0
    rc, err = _call(first, last, regs, C.byref(s), keep=65)
    assert rc == capi.DVT_ERR_INPUT and "cap_each 65" in err
    assert _call(first, last, regs, C.byref(s), keep=64)[0] == capi.DVT_OK
    rc, err = _call(first, last, regs, C.byref(s), window=16385)
    assert rc == capi.DVT_ERR_INPUT and "window 16385" in err
    assert _call(first, last, regs, C.byref(s), window=16384, flags=capi.DVT_DIVERGE_REJOIN)[0] == capi.DVT_OK and s.window == 16384
    assert _call(first, last, regs, C.byref(s), flags=2)[0] == capi.DVT_ERR_INPUT
    assert _call(first, last, regs, C.byref(s), log_shard=23)[0] == capi.DVT_ERR_INPUT


def test_a_start_past_the_end_is_the_end():
    cycles = capi.execute_diverge(ELF, A, B)[2]["summary"]["cycles_a"]
    for start in ((1, cycles), (1, 1 << 20), (2, 0), (9, 9)):      # positions compare as pairs, as the snapshot's do
        rc, reps, got, err = capi.execute_diverge(ELF, A, B, start_a=start)
        assert rc == capi.DVT_OK and got["summary"]["n_pairs"] == 0 and got["summary"]["reason"] == capi.DVT_DIV_END_A, (start, err)
        assert got["summary"]["stop_a"] is None and got["summary"]["stop_b"]["idx"] == 0 and got["summary"]["prev_a"] is None
        assert (got["summary"]["stop_shard_a"], got["summary"]["stop_row_a"]) == (1, cycles)
    rc, reps, got, err = capi.execute_diverge(ELF, A, B, start_a=(0, 5), start_b=(1, 0))
    assert rc == capi.DVT_OK and got["summary"]["n_pairs"] == cycles, err
