"""The ABI of the execution report without a GPU: the two symbols are exported with everything else the header declares, the
ABI version moved to 12, the four structs have the header's sizes, and the entries refuse NULL arguments."""
import ctypes as C
import os
import re

from dvt_circuits_amd import capi
from tests import guests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_profile_symbols_are_exported_with_the_rest():
    lib = capi.load()
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(dvt_[a-z0-9_]+)\s*\(", src))
    assert {"dvt_rv32_job_profile", "dvt_execute_profile"} <= names
    for name in sorted(names):
        assert hasattr(lib, name), name


def test_abi_version_is_at_least_12():
    assert capi.load().dvt_abi_version() >= 12


def test_structs_match_the_header():
    # dvt_profile_edge: 2 x u32 + u64; dvt_profile_syscall: 2 x u32 + u64; dvt_profile_opcode: char[8] + u64;
    # dvt_profile_summary: 3 x u64 + 7 x u32 + float
    assert C.sizeof(capi.ProfileEdge) == 16 and C.sizeof(capi.ProfileSyscall) == 16 and C.sizeof(capi.ProfileOpcode) == 16
    assert C.sizeof(capi.ProfileSummary) == 56 and capi.ProfileSummary.ms.offset == 52 and capi.ProfileSummary.text_base.offset == 24
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dvt_profile_summary;", src).group(1)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert fields == [name for name, _ in capi.ProfileSummary._fields_]


def test_null_arguments_are_input_errors():
    lib = capi.load()
    s = capi.ProfileSummary()
    none = (None, 0, None, 0, None, 0, None, 0)
    assert lib.dvt_rv32_job_profile(None, None, None, 0, *none, C.byref(s)) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_job_profile(None, None, None, 0, *none, None) == capi.DVT_ERR_INPUT
    elf = guests.exit_with(0)
    rep, err = capi.Report(), C.c_char_p()
    assert lib.dvt_execute_profile(elf, len(elf), None, 0, 0, *none, None, C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert lib.dvt_execute_profile(None, 0, None, 0, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    # an array that is NULL with a cap
    assert lib.dvt_execute_profile(elf, len(elf), None, 0, 0, None, 4, None, 0, None, 0, None, 0, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    # and the sizes alone
    assert lib.dvt_execute_profile(elf, len(elf), None, 0, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_OK
    assert s.n_instr == len(elf[52 + 32:]) // 4 and s.cycles == rep.cycles and s.n_syscalls == 1 and s.n_edges == 0
