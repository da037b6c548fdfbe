"""The ABI of the call-tree report without a GPU: the symbols are exported, the ABI version moved to 14, the three structs have
the header's layout, the entries refuse NULL arguments and bad caps, and the size query works."""
import ctypes as C
import os
import re

from dvt_circuits_amd import capi
from tests import guests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calltree_symbols_are_exported_with_the_rest():
    lib = capi.load()
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(dvt_[a-z0-9_]+)\s*\(", src))
    assert {"dvt_rv32_job_calltree", "dvt_rv32_job_calltree_times", "dvt_execute_calltree"} <= names
    for name in sorted(names):
        assert hasattr(lib, name), name


def test_abi_version_is_at_least_14():
    assert capi.load().dvt_abi_version() >= 14


def test_structs_match_the_header():
    # dvt_calltree_arc: 2 x u32 + 2 x u64; dvt_calltree_func: 2 x u32 + 3 x u64; dvt_calltree_summary: 5 x u64 + 7 x u32 + float
    assert C.sizeof(capi.CalltreeArc) == 24 and C.sizeof(capi.CalltreeFunc) == 32 and C.sizeof(capi.CalltreeSummary) == 72
    assert capi.CalltreeSummary.text_base.offset == 40 and capi.CalltreeSummary.ms.offset == 68
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    for name, cls in (("arc", capi.CalltreeArc), ("func", capi.CalltreeFunc), ("summary", capi.CalltreeSummary)):
        body = re.search(r"typedef struct \{([^}]*)\} dvt_calltree_%s;" % name, src).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert fields == [n for n, _ in cls._fields_], name


def test_null_arguments_and_caps_are_input_errors():
    lib = capi.load()
    s = capi.CalltreeSummary()
    none = (None, 0, None, 0)
    assert lib.dvt_rv32_job_calltree(None, None, None, 0, *none, C.byref(s)) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_job_calltree(None, None, None, 0, *none, None) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_job_calltree_times(None, None) == capi.DVT_ERR_INPUT
    elf = guests.exit_with(0)
    rep, err = capi.Report(), C.c_char_p()
    assert lib.dvt_execute_calltree(elf, len(elf), None, 0, 0, *none, None, C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert lib.dvt_execute_calltree(None, 0, None, 0, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    # an array that is NULL with a cap
    assert lib.dvt_execute_calltree(elf, len(elf), None, 0, 0, None, 4, None, 0, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert lib.dvt_execute_calltree(elf, len(elf), None, 0, 0, None, 0, None, 1, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    # something that is no ELF
    assert lib.dvt_execute_calltree(b"junk", 4, None, 0, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert err.value
    lib.dvt_free(C.cast(err, C.c_void_p))


def test_the_size_query_and_short_arrays():
    lib = capi.load()
    elf = guests.exit_with(0)
    s, rep, err = capi.CalltreeSummary(), capi.Report(), C.c_char_p()
    assert lib.dvt_execute_calltree(elf, len(elf), None, 0, 0, None, 0, None, 0, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_OK
    # a guest without a call: the root alone
    assert (s.n_arcs, s.n_funcs, s.n_frames, s.max_depth, s.open_at_exit, s.unmatched_returns) == (1, 1, 1, 1, 1, 0)
    assert s.n_instr == len(elf[52 + 32:]) // 4 and s.cycles == rep.cycles and s.shards_total == 1
    arcs, funcs = (capi.CalltreeArc * 1)(), (capi.CalltreeFunc * 1)()
    assert lib.dvt_execute_calltree(elf, len(elf), None, 0, 0, arcs, 1, funcs, 1, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_OK
    assert (arcs[0].caller_pc, arcs[0].callee_pc, arcs[0].calls, arcs[0].cycles) == (0xffffffff, s.text_base, 1, rep.cycles)
    assert (funcs[0].pc, funcs[0].calls, funcs[0].inclusive, funcs[0].self) == (s.text_base, 1, rep.cycles, rep.cycles)
    # caps below the sizes: the first entries, and the summary still counts all
    from tests import guests_calltree
    elf = guests_calltree.tail()
    rc, _, whole, _ = capi.execute_calltree(elf)
    assert rc == 0 and whole["summary"]["n_arcs"] > 2
    arcs = (capi.CalltreeArc * 2)()
    assert lib.dvt_execute_calltree(elf, len(elf), None, 0, 0, arcs, 2, None, 0, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_OK
    assert s.n_arcs == whole["summary"]["n_arcs"] and s.n_funcs == whole["summary"]["n_funcs"]
    assert [(a.caller_pc, a.callee_pc, a.calls, a.cycles) for a in arcs] == [tuple(a) for a in whole["arcs"][:2]]
