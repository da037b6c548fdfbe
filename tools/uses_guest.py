#!/usr/bin/env python3
"""Who reads a value of a guest's execution, and what those readers produce: the forward data-flow slice of a register or a
memory word from a position on, as an indented tree (dvt_rv32_job_uses on the GPU, dvt_execute_uses with --host; the rule is
stated in csrc/uses.h).

    python tools/uses_guest.py --guest 'bignum(40)' --at 3:0 --reg a3 [--depth N] [--fan N] [--nodes N] [--follow-addr] [--host]
    python tools/uses_guest.py --guest 'sub_stores()' --at 1:0 --word 0x300010 [--log-shard L]
    python tools/uses_guest.py --elf guest.elf [--stdin FILE ...] --at 2:100 --reg a0

--at S:R is the position of an instruction as the watchpoints print it: the value the register or word holds when that
instruction begins is followed.  One line per definition: the register or word, its value (?? when the records do not hold it:
the words a precompile call wrote), the exact number of its uses and its next writer (`live` when nothing writes it again);
under it its first --fan uses, each named by the role it reads the value in (rs1 / rs2 / addr / mem) and its consumer: depth,
SHARD:ROW, pc, kind and values; under a consumer the definitions it makes.  A consumer that was printed before comes back as a
reference (^ SHARD:ROW); `cut -> SHARD:ROW` names a consumer the node limit left out; `...` marks a consumer whose definitions
were not followed (--depth, or the definition or edge limit); `+N more` the uses beyond --fan.  The summary line comes first.

--from-diverge is not offered: the tool takes the position and the operand from the command line, and a divergence report is
printed by tools/diverge_guest.py, whose differing operand (shard, row and the register of the instruction) can be passed here
as --at and --reg."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.origin_guest import KINDS, format_node, parse_target  # noqa: E402,F401
from tools.profile_guest import guest_elf  # noqa: E402
from tools.snapshot_guest import ABI, parse_at  # noqa: E402

NONE = 0xFFFFFFFF
REG, WORD = 1, 2
ROLES = {1: "addr", 2: "rs1", 3: "rs2", 4: "mem"}
LIVE_AT_EXIT, TRUNCATED, NO_VALUE, CUT, UNEXPANDED = 1, 2, 4, 8, 16


def format_def(d):
    name = ABI[d["target"]] if d["what"] == REG else "[0x%08x]" % d["target"]
    value = "??" if d["flags"] & NO_VALUE else "0x%08x" % d["value"]
    ends = "live" if d["flags"] & LIVE_AT_EXIT else "until %d:%d" % (d["next_shard"], d["next_row"])
    return "%s = %s, %d use%s, %s" % (name, value, d["n_uses"], "" if d["n_uses"] == 1 else "s", ends)


def format_uses(got):
    """the lines of a slice (capi's dict): the summary, then the tree from the root definition"""
    s = got["summary"]
    where = "after the last instruction" if s["position"] == s["cycles"] else "from %d:%d" % (s["shard"], s["row"])
    lines = ["%s (instruction %d of %d): %d nodes, %d definitions, %d edges, depth %d; %d cut, %d unexpanded, %d truncated, %d dead, %d live at the exit, "
             "%d without a value; %d uses in all; %d levels, %d passes" % (where, s["position"], s["cycles"], s["n_nodes"], s["n_defs"], s["n_edges"], s["depth"],
                                                                            s["cut"], s["unexpanded"], s["truncated"], s["dead"], s["live_at_exit"], s["no_value"],
                                                                            s["uses_total"], s["levels"], s["passes"])]
    seen = set()
    stack = [("def", 0, 0)]      # depth first: the uses of a definition in execution order, the definitions of a consumer in theirs
    while stack:
        kind, k, indent = stack.pop()
        pad = "  " * indent
        if kind == "def":
            d = got["defs"][k]
            more = d["n_uses"] - d["n_edges"]
            lines.append("%s%s%s" % (pad, format_def(d), " (+%d more)" % more if more else ""))
            stack += [("edge", e, indent + 1) for e in reversed(range(d["first_edge"], d["first_edge"] + d["n_edges"]))]
            continue
        e = got["edges"][k]
        head = "%s%s -> " % (pad, ROLES[e["role"]])
        if e["to"] == NONE:
            lines.append(head + "cut -> %d:%d" % (e["dst_shard"], e["dst_row"]))
            continue
        n = got["nodes"][e["to"]]
        if e["to"] in seen:
            lines.append(head + "^ %d:%d" % (n["shard"], n["row"]))
            continue
        seen.add(e["to"])
        lines.append(head + "%d %s%s" % (n["depth"], format_node(n), " ..." if n["flags"] & UNEXPANDED else ""))
        stack += [("def", j, indent + 1) for j in reversed(range(n["first_def"], n["first_def"] + n["n_defs"]))]
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
    ap.add_argument("--fan", type=int, default=8)
    ap.add_argument("--nodes", type=int, default=1024)
    ap.add_argument("--follow-addr", action="store_true", help="also follow the address registers of loads and stores")
    ap.add_argument("--host", action="store_true", help="on the host (dvt_execute_uses): no GPU is touched")
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
        rc, rep, got, err = capi.execute_uses(elf, stdin, at, target, args.follow_addr, args.depth, args.fan, args.nodes, log_shard=args.log_shard)
        if got is None:
            raise SystemExit("uses failed: %s" % err)
        if err:
            print("the guest failed: %s" % err)
    else:
        p = capi.Prover('{"log_shard_size": %d}' % args.log_shard)
        pk, _ = p.setup(elf)
        job, rep = p.prepare(pk, stdin)
        got = p.job_uses(pk, job, at, target, args.follow_addr, args.depth, args.fan, args.nodes)
        print("next %.3f ms, count %.3f ms, emit %.3f ms, gather %.3f ms, host %.3f ms" % tuple(
            p.job_uses_times()[k] for k in ("next_ms", "count_ms", "emit_ms", "gather_ms", "host_ms")))
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    for line in format_uses(got):
        print(line)


if __name__ == "__main__":
    main()
