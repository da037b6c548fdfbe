"""The ABI of the memory report without a GPU: the symbols are exported, the ABI version moved to 15, the two structs have the
header's layout, the entries refuse NULL arguments and bad caps, and the size query works."""
import ctypes as C
import os
import re

from dvt_circuits_amd import capi
from tests import guests, guests_memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_memory_symbols_are_exported_with_the_rest():
    lib = capi.load()
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(dvt_[a-z0-9_]+)\s*\(", src))
    assert {"dvt_rv32_job_memory", "dvt_execute_memory"} <= names
    for name in sorted(names):
        assert hasattr(lib, name), name


def test_abi_version_is_at_least_15():
    assert capi.load().dvt_abi_version() >= 15


def test_structs_match_the_header():
    # dvt_memory_page: 4 x u32 + 4 x u64; dvt_memory_summary: 12 x u64 + 8 x u32 + float, padded to a multiple of 8
    assert C.sizeof(capi.MemoryPage) == 48 and C.sizeof(capi.MemorySummary) == 136
    assert capi.MemoryPage.loads.offset == 16 and capi.MemorySummary.sp_min.offset == 96 and capi.MemorySummary.ms.offset == 128
    src = open(os.path.join(ROOT, "include", "dvt_prover.h")).read()
    for name, cls in (("page", capi.MemoryPage), ("summary", capi.MemorySummary)):
        body = re.search(r"typedef struct \{([^}]*)\} dvt_memory_%s;" % name, src).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert fields == [n for n, _ in cls._fields_], name


def test_the_page_cache_constant_is_the_sources():
    src = open(os.path.join(ROOT, "dvt_circuits_amd", "csrc", "memreport.h")).read()
    assert int(re.search(r"LDS_PAGE_SLOTS = (\d+);", src).group(1)) == capi.MEMORY_LDS_PAGE_SLOTS


def test_null_arguments_and_caps_are_input_errors():
    lib = capi.load()
    s = capi.MemorySummary()
    none = (None, 0, None, 0)
    assert lib.dvt_rv32_job_memory(None, None, None, *none, C.byref(s)) == capi.DVT_ERR_INPUT
    assert lib.dvt_rv32_job_memory(None, None, None, *none, None) == capi.DVT_ERR_INPUT
    elf = guests.exit_with(0)
    rep, err = capi.Report(), C.c_char_p()
    assert lib.dvt_execute_memory(elf, len(elf), None, 0, 0, *none, None, C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert lib.dvt_execute_memory(None, 0, None, 0, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert lib.dvt_execute_memory(elf, len(elf), None, 1, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    # an array that is NULL with a cap
    assert lib.dvt_execute_memory(elf, len(elf), None, 0, 0, None, 4, None, 0, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert lib.dvt_execute_memory(elf, len(elf), None, 0, 0, None, 0, None, 1, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    # something that is no ELF
    assert lib.dvt_execute_memory(b"junk", 4, None, 0, 0, *none, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_ERR_INPUT
    assert err.value
    lib.dvt_free(C.cast(err, C.c_void_p))


def test_the_size_query_and_short_arrays():
    lib = capi.load()
    elf = guests.exit_with(0)
    s, rep, err = capi.MemorySummary(), capi.Report(), C.c_char_p()
    assert lib.dvt_execute_memory(elf, len(elf), None, 0, 0, None, 0, None, 0, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_OK
    # a guest without a load or a store: no page, and the image alone in mem_init
    assert (s.n_pages, s.words, s.loads, s.stores, s.first_touches, s.pre_calls, s.sp_writes, s.sp_min, s.sp_max) == (0,) * 9
    assert s.n_instr == len(elf[52 + 32:]) // 4 <= s.image_words and s.cycles == rep.cycles and s.shards_total == s.shards_tallied == 1
    assert s.mem_init_rows == 32 + s.image_words and s.page_bytes == 4096
    # caps below the sizes: the first entries, and the summary still counts all
    elf = guests_memory.many_pages()
    rc, _, whole, _ = capi.execute_memory(elf)
    assert rc == 0 and whole["summary"]["n_pages"] > 300
    pages, ft = (capi.MemoryPage * 2)(), (C.c_uint64 * 3)()
    assert lib.dvt_execute_memory(elf, len(elf), None, 0, 0, ft, 3, pages, 2, C.byref(s), C.byref(rep), C.byref(err)) == capi.DVT_OK
    assert s.n_pages == whole["summary"]["n_pages"] and s.n_instr == whole["summary"]["n_instr"] > 3
    assert [(pg.page, pg.words, pg.first, pg.loads, pg.stores) for pg in pages] == \
        [(pg["page"], pg["words"], pg["first"], pg["loads"], pg["stores"]) for pg in whole["pages"][:2]]
    assert list(ft) == [int(x) for x in whole["first_touch"][:3]]
