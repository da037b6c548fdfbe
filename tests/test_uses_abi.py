"""The uses entry points of the C ABI (no GPU): they exist, the structs have the sizes of include/dvt_prover.h, the constants of
capi.py are the header's, every input error of the rule is refused with DVT_ERR_INPUT and its text, and the limits are the ones
stated."""
import ctypes as C
import os

import pytest

from dvt_circuits_amd import capi
from tests import guests

ELF = guests.arith()[0]
ADDR_LIMIT = 0x38000000
BASE = 0x400000
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvt_prover.h")).read()


def test_entry_points_sizes_and_version():
    lib = capi.load()
    assert lib.dvt_abi_version() >= 21
    for name in ("dvt_rv32_job_uses", "dvt_rv32_job_uses_times", "dvt_execute_uses"):
        assert hasattr(lib, name), name
    assert (C.sizeof(capi.UsesNode), C.sizeof(capi.UsesDef), C.sizeof(capi.UsesEdge), C.sizeof(capi.UsesSummary)) == (64, 48, 24, 96)
    for name, value in (("MAX_NODES", 1024), ("MAX_DEFS", 4096), ("MAX_EDGES", 8192), ("MAX_DEPTH", 64), ("MAX_FAN", 16), ("DEFAULT_FAN", 8), ("PASS_DEFS", 256),
                        ("SPAN", 4096)):
        assert getattr(capi, "DVT_USES_" + name) == value, name
        assert any(line.split()[:3] == ["#define", "DVT_USES_" + name, str(value)] for line in HEADER.splitlines()), name
    assert "#define DVT_USES_NONE 0xffffffffu" in HEADER and capi.DVT_USES_NONE == 0xFFFFFFFF
    for line in ("enum { DVT_USES_REG = 1, DVT_USES_WORD = 2 };", "enum { DVT_USES_FOLLOW_ADDR = 1 };",
                 "enum { DVT_USES_OP = 1, DVT_USES_LOAD = 2, DVT_USES_STORE = 3, DVT_USES_CALL = 4, DVT_USES_SYSCALL = 5 };",
                 "enum { DVT_USES_ADDR = 1, DVT_USES_RS1 = 2, DVT_USES_RS2 = 3, DVT_USES_MEM = 4 };",
                 "enum { DVT_USES_LIVE_AT_EXIT = 1, DVT_USES_TRUNCATED = 2, DVT_USES_NO_VALUE = 4, DVT_USES_CUT = 8, DVT_USES_UNEXPANDED = 16 };"):
        assert line in HEADER, line
    assert (capi.DVT_USES_REG, capi.DVT_USES_WORD, capi.DVT_USES_FOLLOW_ADDR) == (1, 2, 1)
    assert (capi.DVT_USES_OP, capi.DVT_USES_LOAD, capi.DVT_USES_STORE, capi.DVT_USES_CALL, capi.DVT_USES_SYSCALL) == (1, 2, 3, 4, 5)
    assert (capi.DVT_USES_ADDR, capi.DVT_USES_RS1, capi.DVT_USES_RS2, capi.DVT_USES_MEM) == (1, 2, 3, 4)
    assert (capi.DVT_USES_LIVE_AT_EXIT, capi.DVT_USES_TRUNCATED, capi.DVT_USES_NO_VALUE, capi.DVT_USES_CUT, capi.DVT_USES_UNEXPANDED) == (1, 2, 4, 8, 16)
    # the field order of the mirrors is the header's
    for cls, name in ((capi.UsesNode, "dvt_uses_node"), (capi.UsesEdge, "dvt_uses_edge")):
        fields = ", ".join(f for f, _ in cls._fields_)
        assert "typedef struct { uint32_t %s; } %s;" % (fields, name) in HEADER, name
    flat = " ".join(HEADER.split())
    assert "typedef struct { uint64_t n_uses; uint32_t %s; } dvt_uses_def;" % ", ".join(f for f, _ in capi.UsesDef._fields_[1:]) in flat
    u64 = [f for f, t in capi.UsesSummary._fields_ if t is C.c_uint64]
    u32 = [f for f, t in capi.UsesSummary._fields_ if t is C.c_uint32 and f != "pad"]
    assert "typedef struct { uint64_t %s; uint32_t %s; float ms;" % (", ".join(u64), ", ".join(u32)) in flat
    assert capi.uses_reg("a0") == (1, 10) and capi.uses_reg(31) == (1, 31) and capi.uses_word(BASE + 7) == (2, BASE + 4)


BAD = {
    "register 0": (dict(target=(capi.DVT_USES_REG, 0)), "register 0 outside 1..31"),
    "register 32": (dict(target=(capi.DVT_USES_REG, 32)), "register 32 outside 1..31"),
    "a misaligned word": (dict(target=(capi.DVT_USES_WORD, BASE + 2)), "word address not 4-aligned"),
    "a word at the address limit": (dict(target=(capi.DVT_USES_WORD, ADDR_LIMIT)), "word address at or past the address limit"),
    "a word above the address limit": (dict(target=(capi.DVT_USES_WORD, 0xFFFFFF00)), "word address at or past the address limit"),
    "an unknown kind of target": (dict(target=(3, 10)), "unknown target kind 3"),
    "kind 0": (dict(target=(0, 10)), "unknown target kind 0"),
    "fan 0": (dict(fan=0), "fan 0 (1..16)"),
    "fan 17": (dict(fan=17), "fan 17 (1..16)"),
    "1025 nodes": (dict(nodes=1025), "cap_nodes 1025 (at most 1024)"),
    "4097 definitions": (dict(defs=4097), "cap_defs 4097 (1..4096)"),
    "no definition": (dict(defs=0), "cap_defs 0 (1..4096)"),
    "8193 edges": (dict(edges=8193), "cap_edges 8193 (fan..8192)"),
    "fewer edges than fan": (dict(edges=7), "cap_edges 7 (fan..8192)"),
    "depth 65": (dict(depth=65), "max_depth 65 (at most 64)"),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_input_errors_are_refused(what):
    kw, text = BAD[what]
    rc, rep, got, err = capi.execute_uses(ELF, [], (1, 0), **kw)
    assert rc == capi.DVT_ERR_INPUT and got is None and err == text, (what, rc, err)
    assert rep["cycles"] == 0    # (refused before the guest runs)


def test_null_arrays_flags_and_shard_sizes_are_refused():
    lib = capi.load()
    nodes, defs, edges, s = (capi.UsesNode * 8)(), (capi.UsesDef * 64)(), (capi.UsesEdge * 64)(), capi.UsesSummary()
    rep, err = capi.Report(), C.c_char_p()

    row, reg = next((r, k) for r in range(1, 64) for k in range(1, 32) if capi.execute_uses(ELF, [], (1, r), capi.uses_reg(k))[2]["edges"])      # a live value

    def call(nodes, cap_nodes, defs, cap_defs, edges, cap_edges, s, flags=0, log_shard=0):
        return lib.dvt_execute_uses(ELF, len(ELF), None, 0, 0, log_shard, 1, row, capi.DVT_USES_REG, reg, flags, 4, 8, nodes, cap_nodes, defs, cap_defs, edges,
                                    cap_edges, s, C.byref(rep), C.byref(err))
    assert call(nodes, 8, defs, 64, edges, 64, C.byref(s)) == capi.DVT_OK and s.cycles == rep.cycles and 1 <= s.n_defs <= 64 and s.n_nodes <= 8
    assert 1 <= s.n_edges <= 64 and s.position == row
    for bad in ((None, 8, defs, 64, edges, 64, C.byref(s)), (nodes, 8, None, 64, edges, 64, C.byref(s)), (nodes, 8, defs, 64, None, 64, C.byref(s))):
        assert call(*bad) == capi.DVT_ERR_INPUT and err.value == b"null array"
        lib.dvt_free(err)
    assert call(nodes, 8, defs, 64, edges, 64, None) == capi.DVT_ERR_INPUT
    assert call(nodes, 8, defs, 64, edges, 64, C.byref(s), flags=2) == capi.DVT_ERR_INPUT and err.value == b"unknown flag"
    lib.dvt_free(err)
    assert call(nodes, 8, defs, 64, edges, 64, C.byref(s), log_shard=23) == capi.DVT_ERR_INPUT
    lib.dvt_free(err)
    # no node array is needed for no nodes: every kept use is then cut, and names its consumer
    assert call(None, 0, defs, 64, edges, 64, C.byref(s)) == capi.DVT_OK and s.n_nodes == 0 and s.n_defs == 1 and s.cut == s.n_edges >= 1
    assert edges[0].flags == capi.DVT_USES_CUT and edges[0].to == capi.DVT_USES_NONE and edges[0].dst_shard == 1


def test_the_limits_are_reached():
    rc, rep, got, err = capi.execute_uses(ELF, [], (1, 0), capi.uses_reg(2), follow_addr=True, depth=64, fan=16, nodes=1024, defs=4096, edges=8192)
    assert rc == capi.DVT_OK, err
    rc, rep, got, err = capi.execute_uses(ELF, [], (1, 0), capi.uses_word(ADDR_LIMIT - 4), fan=1, edges=1)
    assert rc == capi.DVT_OK and got["nodes"] == [] and got["edges"] == [] and len(got["defs"]) == 1, err
    root = got["defs"][0]
    assert root["flags"] == capi.DVT_USES_LIVE_AT_EXIT | capi.DVT_USES_NO_VALUE and root["node"] == root["next_shard"] == root["next_row"] == capi.DVT_USES_NONE
    assert got["summary"]["dead"] == got["summary"]["live_at_exit"] == got["summary"]["no_value"] == 1


def test_the_summary_of_a_call():
    rc, rep, got, err = capi.execute_uses(ELF, [], (2, 5), capi.uses_reg("a0"), log_shard=10)
    s = got["summary"]
    assert rc == capi.DVT_OK and s["cycles"] == rep["cycles"] and s["shards_total"] == (rep["cycles"] + 1023) // 1024, err
    assert (s["position"], s["shard"], s["row"], s["span"], s["passes"]) == (1024 + 5, 2, 5, capi.DVT_USES_SPAN, 0)
    assert s["n_nodes"] == len(got["nodes"]) and s["n_defs"] == len(got["defs"]) >= 1 and s["n_edges"] == len(got["edges"]) and s["levels"] >= 1
    assert s["uses_total"] == sum(d["n_uses"] for d in got["defs"])
    # the exit has no uses, whatever its spelling
    end = capi.execute_uses(ELF, [], capi.SNAP_EXIT, capi.uses_reg("a0"), log_shard=10)[2]
    far = capi.execute_uses(ELF, [], (s["shards_total"] + 3, 0), capi.uses_reg("a0"), log_shard=10)[2]
    assert end["nodes"] == far["nodes"] == [] and end["defs"] == far["defs"] and end["defs"][0]["n_uses"] == 0
    assert end["summary"]["position"] == far["summary"]["position"] == rep["cycles"]
