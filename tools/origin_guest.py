#!/usr/bin/env python3
"""Where a value of a guest's execution comes from: the backward data-flow slice of a register or a memory word at a position,
as an indented tree (dvt_rv32_job_origin on the GPU, dvt_execute_origin with --host; the rule is stated in csrc/origin.h).

    python tools/origin_guest.py --guest 'bignum(40)' --at exit --reg a1 [--depth N] [--nodes N] [--follow-addr] [--host]
    python tools/origin_guest.py --guest 'sub_stores()' --at 3:480 --word 0x300010 [--log-shard L]
    python tools/origin_guest.py --elf guest.elf [--stdin FILE ...] --at exit --reg a0

--at S:R is the position of an instruction as the watchpoints print it; `exit` is the state after the last instruction, of a
guest that traps (with --host) the state at the trap.  One line per node: its depth, SHARD:ROW, pc, kind and values; under it
its inputs, each named by its role (rs1 / rs2 / addr / mem), its register or word and the value the record read.  A node that
was printed before comes back as a reference (^ SHARD:ROW); a leaf prints as `initial` (nothing wrote the register or word
before), `image` (an initial word of the program image) or `cut -> SHARD:ROW` (the node limit was reached: the producer is
named but not followed); `...` marks a node whose inputs were not followed (--depth, or the edge limit).  ?? stands for a value
the records do not hold (the words of a precompile call).  The summary line comes first."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.profile_guest import guest_elf  # noqa: E402
from tools.snapshot_guest import ABI, parse_at  # noqa: E402,F401

NONE = 0xFFFFFFFF
REG, WORD = 1, 2
KINDS = {1: "op", 2: "load", 3: "store", 4: "call", 5: "syscall"}
ROLES = {0: "root", 1: "addr", 2: "rs1", 3: "rs2", 4: "mem"}
INITIAL, IMAGE, NO_VALUE, CUT, UNEXPANDED = 1, 2, 4, 8, 16


def parse_target(reg, word):
    """(what, target) of --reg NAME (x1..x31 or an ABI name) or --word ADDR"""
    if (reg is None) == (word is None):
        raise ValueError("one of --reg and --word")
    if reg is not None:
        k = ABI.index(reg) if reg in ABI else int(reg[1:]) if reg[:1] == "x" and reg[1:].isdigit() else 0
        if not 1 <= k <= 31:
            raise ValueError("no register (x1..x31 or an ABI name): %r" % reg)
        return REG, k
    return WORD, int(word, 0) & ~3


def _name(e, what):
    if e["role"] == 4 or (e["role"] == 0 and what == WORD):
        return "[0x%08x]" % e["target"]
    return ABI[e["target"]]


def _value(e):
    return "??" if e["flags"] & NO_VALUE else "0x%08x" % e["value"]


def format_node(n):
    text = "%d:%d pc 0x%08x %-7s rd 0x%08x rs1 0x%08x rs2 0x%08x" % (n["shard"], n["row"], n["pc"], KINDS.get(n["kind"], "?"), n["rd_value"], n["rs1"], n["rs2"])
    if n["kind"] in (2, 3):
        text += " [0x%08x] 0x%08x -> 0x%08x" % (n["addr"], n["before"], n["after"])
    return text


def format_origin(got, what):
    """the lines of a slice (capi's dict): the summary, then the tree from the root"""
    s = got["summary"]
    where = "after the last instruction" if s["position"] == s["cycles"] else "before %d:%d" % (s["shard"], s["row"])
    lines = ["%s (instruction %d of %d): %d nodes, %d edges, depth %d; %d cut, %d unexpanded, %d initial, %d without a value; %d questions in %d levels, "
             "%d passes" % (where, s["position"], s["cycles"], s["n_nodes"], s["n_edges"], s["depth"], s["cut"], s["unexpanded"], s["initial"], s["no_value"],
                            s["questions"], s["levels"], s["passes"])]
    seen = set()
    stack = [(0, 0)]      # (edge, indent): depth first, the inputs of a node in their order
    while stack:
        ei, indent = stack.pop()
        e = got["edges"][ei]
        head = "%s%s %s = %s <- " % ("  " * indent, ROLES[e["role"]], _name(e, what), _value(e))
        if e["to"] == NONE:
            leaf = "cut -> %d:%d" % (e["src_shard"], e["src_row"]) if e["flags"] & CUT else "image" if e["flags"] & IMAGE else "initial"
            lines.append(head + leaf)
            continue
        n = got["nodes"][e["to"]]
        if e["to"] in seen:
            lines.append(head + "^ %d:%d" % (n["shard"], n["row"]))
            continue
        seen.add(e["to"])
        lines.append(head + "%d %s%s" % (n["depth"], format_node(n), " ..." if n["flags"] & UNEXPANDED else ""))
        stack += [(k, indent + 1) for k in reversed(range(n["first_edge"], n["first_edge"] + n["n_edges"]))]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--guest")
    ap.add_argument("--elf")
    ap.add_argument("--stdin", action="append", default=[])
    ap.add_argument("--at", required=True, metavar="S:R|exit")
    ap.add_argument("--reg", metavar="NAME")
    ap.add_argument("--word", metavar="ADDR")
    ap.add_argument("--depth", type=int, default=64)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--follow-addr", action="store_true", help="also follow the address registers of loads and stores")
    ap.add_argument("--host", action="store_true", help="on the host (dvt_execute_origin): no GPU is touched")
    ap.add_argument("--log-shard", type=int, default=21)
    args = ap.parse_args()
    if bool(args.guest) == bool(args.elf):
        ap.error("one of --guest and --elf")
    try:
        target, at = parse_target(args.reg, args.word), parse_at(args.at)
    except ValueError as e:
        ap.error(str(e))
    from dvt_circuits_amd import capi

    elf = guest_elf(args.guest) if args.guest else open(args.elf, "rb").read()
    stdin = [open(f, "rb").read() for f in args.stdin]
    if args.host:
        rc, rep, got, err = capi.execute_origin(elf, stdin, at, target, args.follow_addr, args.depth, args.nodes, log_shard=args.log_shard)
        if got is None:
            raise SystemExit("origin failed: %s" % err)
        if err:
            print("the guest failed: %s" % err)
    else:
        p = capi.Prover('{"log_shard_size": %d}' % args.log_shard)
        pk, _ = p.setup(elf)
        job, rep = p.prepare(pk, stdin)
        got = p.job_origin(pk, job, at, target, args.follow_addr, args.depth, args.nodes)
        print("reduce %.3f ms, gather %.3f ms, host %.3f ms" % tuple(p.job_origin_times()[k] for k in ("reduce_ms", "gather_ms", "host_ms")))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    for line in format_origin(got, target[0]):
        print(line)


if __name__ == "__main__":
    main()
