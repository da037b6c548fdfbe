"""The origin entry points of the C ABI (no GPU): they exist, the structs have the sizes of include/dvt_prover.h, every input
error of the rule is refused with DVT_ERR_INPUT and a text, and the limits are the ones stated."""
import ctypes as C
import os

import pytest

from dvt_circuits_amd import capi
from tests import guests

ELF = guests.arith()[0]
ADDR_LIMIT = 0x38000000
BASE = 0x400000


def test_entry_points_sizes_and_version():
    lib = capi.load()
    assert lib.dvt_abi_version() >= 19
    for name in ("dvt_rv32_job_origin", "dvt_rv32_job_origin_times", "dvt_execute_origin"):
        assert hasattr(lib, name), name
    assert (C.sizeof(capi.OriginNode), C.sizeof(capi.OriginEdge), C.sizeof(capi.OriginSummary)) == (64, 32, 80)
    assert (capi.DVT_ORIGIN_MAX_NODES, capi.DVT_ORIGIN_MAX_EDGES, capi.DVT_ORIGIN_MAX_DEPTH, capi.DVT_ORIGIN_PASS_QUESTIONS, capi.DVT_ORIGIN_SPAN) == \
        (1024, 8192, 64, 256, 4096)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvt_prover.h")).read()
    for line in ("#define DVT_ORIGIN_MAX_NODES 1024", "#define DVT_ORIGIN_MAX_EDGES 8192", "#define DVT_ORIGIN_MAX_DEPTH 64",
                 "#define DVT_ORIGIN_PASS_QUESTIONS 256", "#define DVT_ORIGIN_SPAN 4096", "#define DVT_ORIGIN_NONE 0xffffffffu",
                 "enum { DVT_ORIGIN_REG = 1, DVT_ORIGIN_WORD = 2 };", "enum { DVT_ORIGIN_FOLLOW_ADDR = 1 };",
                 "enum { DVT_ORIGIN_OP = 1, DVT_ORIGIN_LOAD = 2, DVT_ORIGIN_STORE = 3, DVT_ORIGIN_CALL = 4, DVT_ORIGIN_SYSCALL = 5 };",
                 "enum { DVT_ORIGIN_ROOT = 0, DVT_ORIGIN_ADDR = 1, DVT_ORIGIN_RS1 = 2, DVT_ORIGIN_RS2 = 3, DVT_ORIGIN_MEM = 4 };",
                 "enum { DVT_ORIGIN_INITIAL = 1, DVT_ORIGIN_IMAGE = 2, DVT_ORIGIN_NO_VALUE = 4, DVT_ORIGIN_CUT = 8, DVT_ORIGIN_UNEXPANDED = 16 };"):
        assert line in text, line
    # the field order of the mirror is the header's
    for cls, name in ((capi.OriginNode, "dvt_origin_node"), (capi.OriginEdge, "dvt_origin_edge")):
        fields = ", ".join(f for f, _ in cls._fields_)
        assert "typedef struct { uint32_t %s; } %s;" % (fields, name) in text, name
    assert capi.origin_reg("a0") == (1, 10) and capi.origin_reg(31) == (1, 31) and capi.origin_word(BASE + 7) == (2, BASE + 4)


BAD = {
    "register 0": dict(target=(capi.DVT_ORIGIN_REG, 0)),
    "register 32": dict(target=(capi.DVT_ORIGIN_REG, 32)),
    "a misaligned word": dict(target=(capi.DVT_ORIGIN_WORD, BASE + 2)),
    "a word at the address limit": dict(target=(capi.DVT_ORIGIN_WORD, ADDR_LIMIT)),
    "a word above the address limit": dict(target=(capi.DVT_ORIGIN_WORD, 0xFFFFFF00)),
    "an unknown kind of target": dict(target=(3, 10)),
    "kind 0": dict(target=(0, 10)),
    "1025 nodes": dict(nodes=1025),
    "8193 edges": dict(edges=8193),
    "no edge": dict(edges=0),
    "depth 65": dict(depth=65),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_input_errors_are_refused(what):
    rc, rep, got, err = capi.execute_origin(ELF, [], capi.SNAP_EXIT, **BAD[what])
    assert rc == capi.DVT_ERR_INPUT and got is None and err, (what, rc, err)
    assert rep["cycles"] == 0    # (refused before the guest runs)


def test_null_arrays_flags_and_shard_sizes_are_refused():
    lib = capi.load()
    nodes, edges, s = (capi.OriginNode * 8)(), (capi.OriginEdge * 64)(), capi.OriginSummary()
    rep, err = capi.Report(), C.c_char_p()

    def call(nodes, cap_nodes, edges, cap_edges, s, flags=0, log_shard=0):
        return lib.dvt_execute_origin(ELF, len(ELF), None, 0, 0, log_shard, 0xFFFFFFFF, 0xFFFFFFFF, capi.DVT_ORIGIN_REG, 10, flags, 4, nodes, cap_nodes, edges,
                                      cap_edges, s, C.byref(rep), C.byref(err))
    assert call(nodes, 8, edges, 64, C.byref(s)) == capi.DVT_OK and s.cycles == rep.cycles and 1 <= s.n_edges <= 64 and s.n_nodes <= 8
    assert call(None, 8, edges, 64, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(nodes, 8, None, 64, C.byref(s)) == capi.DVT_ERR_INPUT
    assert call(nodes, 8, edges, 64, None) == capi.DVT_ERR_INPUT
    assert call(nodes, 8, edges, 64, C.byref(s), flags=2) == capi.DVT_ERR_INPUT
    assert call(nodes, 8, edges, 64, C.byref(s), log_shard=23) == capi.DVT_ERR_INPUT
    # no node array is needed for no nodes: the root is then cut, and names its writer
    assert call(None, 0, edges, 64, C.byref(s)) == capi.DVT_OK and (s.n_nodes, s.n_edges, s.cut) == (0, 1, 1)
    assert edges[0].flags == capi.DVT_ORIGIN_CUT and edges[0].to == capi.DVT_ORIGIN_NONE and edges[0].src_shard == 1


def test_the_limits_are_reached():
    rc, rep, got, err = capi.execute_origin(ELF, [], capi.SNAP_EXIT, capi.origin_reg(31), depth=64, nodes=1024, edges=8192)
    assert rc == capi.DVT_OK, err
    rc, rep, got, err = capi.execute_origin(ELF, [], capi.SNAP_EXIT, capi.origin_word(ADDR_LIMIT - 4))
    assert rc == capi.DVT_OK and got["nodes"] == [] and len(got["edges"]) == 1, err
    root = got["edges"][0]
    assert root["flags"] == capi.DVT_ORIGIN_INITIAL | capi.DVT_ORIGIN_NO_VALUE and root["to"] == root["from"] == capi.DVT_ORIGIN_NONE


def test_the_summary_of_a_call():
    rc, rep, got, err = capi.execute_origin(ELF, [], (2, 5), capi.origin_reg("a0"), log_shard=10)
    s = got["summary"]
    assert rc == capi.DVT_OK and s["cycles"] == rep["cycles"] and s["shards_total"] == (rep["cycles"] + 1023) // 1024, err
    assert (s["position"], s["shard"], s["row"], s["span"], s["passes"]) == (1024 + 5, 2, 5, capi.DVT_ORIGIN_SPAN, 0)
    assert s["n_nodes"] == len(got["nodes"]) and s["n_edges"] == len(got["edges"]) == s["questions"] and s["levels"] >= 1
    # a position past the end is the end, whatever its spelling
    end = capi.execute_origin(ELF, [], capi.SNAP_EXIT, capi.origin_reg("a0"), log_shard=10)[2]
    far = capi.execute_origin(ELF, [], (s["shards_total"] + 3, 0), capi.origin_reg("a0"), log_shard=10)[2]
    assert end["nodes"] == far["nodes"] and end["edges"] == far["edges"]
    assert end["summary"]["position"] == far["summary"]["position"] == rep["cycles"]
