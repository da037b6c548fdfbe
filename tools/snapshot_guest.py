#!/usr/bin/env python3
"""The machine at one moment of a guest's execution: registers, memory words and the call stack as they are before the
instruction at a position executes (dvt_rv32_job_snapshot on the GPU, dvt_execute_snapshot with --host; the rule is stated in
csrc/snapshot.h).

    python tools/snapshot_guest.py --guest 'recurse()' --at 1:11526 --stack 64 [--frames N] [--host]
    python tools/snapshot_guest.py --guest 'hammer()' --at exit --dump 0x3000e0+64 [--log-shard L]
    python tools/snapshot_guest.py --elf guest.elf [--stdin FILE ...] --at exit

--at S:R is the position of an instruction as the watchpoints print it (shards are numbered from 1, R is the index of the
instruction in its shard); `exit` is the state after the last instruction, of a guest that traps (with --host) the state at
the trap.  --dump ADDR+LEN (repeatable, at most 16, 4096 words in all) shows the words that hold those bytes; --stack N shows N
bytes from the stack pointer of the snapshot, which takes a second call.  A word prints as ?? when the records do not hold its
value (a precompile call wrote it and nothing loads it before the next such write, or nothing ever accessed it and it is no
part of the image), and with a * when nothing accessed it before the position: its value is then the one it started with,
which a hinted word holds only from its HINT_READ on.  Frames are named as tools/profile_guest.py names functions."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.profile_guest import flat_profile, guest_elf  # noqa: E402

INITIAL, FROM_BEFORE, FROM_AFTER, LOAD, STORE, IMAGE, NO_VALUE, UNTOUCHED = 1, 2, 4, 8, 16, 32, 64, 128
EXIT = (0xFFFFFFFF, 0xFFFFFFFF)
ABI = ["zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1"] + ["a%d" % i for i in range(8)] + ["s%d" % i for i in range(2, 12)] + \
      ["t3", "t4", "t5", "t6"]


def parse_at(text):
    """a position: S:R or exit"""
    if text == "exit":
        return EXIT
    s, sep, r = text.partition(":")
    if not sep or not s or not r:
        raise ValueError("no position (S:R or exit): %r" % text)
    return int(s, 0), int(r, 0)


def parse_dump(text):
    """ADDR+LEN as the (lo, hi) range of the words that hold those bytes"""
    a, sep, n = text.partition("+")
    if not sep or int(n, 0) <= 0:
        raise ValueError("no range (ADDR+LEN): %r" % text)
    return int(a, 0) & ~3, (int(a, 0) + int(n, 0) + 3) & ~3


def format_word(c):
    if c["flags"] & NO_VALUE:
        return "      ?? "
    return "%08x%s" % (c["value"], "*" if c["flags"] & INITIAL else " ")


def format_snapshot(snap, ranges, function_of=lambda pc: ""):
    """the lines of a snapshot (capi's dict) with the cells of `ranges` (the ones the snapshot was asked for)"""
    s = snap["summary"]
    where = "after the last instruction" if s["position"] == s["cycles"] else "before %d:%d" % (s["shard"], s["row"])
    lines = ["%s (instruction %d of %d), pc 0x%08x %s" % (where, s["position"], s["cycles"], s["pc"], function_of(s["pc"]))]
    for k in range(1, 32, 4):
        lines.append("  " + "  ".join("%-4s %08x%s" % (ABI[r], snap["regs"][r]["value"], "*" if snap["regs"][r]["flags"] & INITIAL else " ")
                                      for r in range(k, min(k + 4, 32))))
    lines.append("call stack: %d frames%s%s" % (s["depth"], ", the innermost %d shown" % s["n_frames"] if s["n_frames"] < s["depth"] else "",
                                                  ", %d returns found only the root" % s["unmatched_returns"] if s["unmatched_returns"] else ""))
    for k, f in enumerate(snap["frames"]):
        called = "the root" if f["call_pc"] == 0xFFFFFFFF else "called at 0x%08x %s, ra 0x%08x" % (f["call_pc"], function_of(f["call_pc"]), f["ra"])
        lines.append("  #%-3d 0x%08x %-10s since %d:%d, %s" % (k, f["fn_pc"], function_of(f["fn_pc"]), f["open_shard"], f["open_row"], called))
    at = 0
    for lo, hi in ranges:
        for a in range(lo, hi, 16):
            cells = snap["words"][at:at + min(4, (hi - a) // 4)]
            at += len(cells)
            lines.append("  0x%08x: %s" % (a, " ".join(format_word(c) for c in cells)))
    if s["no_value"]:
        lines.append("  ?? : %d words whose value the records do not hold" % s["no_value"])
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--guest")
    ap.add_argument("--elf")
    ap.add_argument("--stdin", action="append", default=[])
    ap.add_argument("--at", required=True, metavar="S:R|exit")
    ap.add_argument("--dump", action="append", default=[], metavar="ADDR+LEN")
    ap.add_argument("--stack", type=int, default=0, metavar="N", help="N bytes from the stack pointer of the snapshot")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--host", action="store_true", help="on the host (dvt_execute_snapshot): no GPU is touched")
    ap.add_argument("--log-shard", type=int, default=21)
    args = ap.parse_args()
    if bool(args.guest) == bool(args.elf):
        ap.error("one of --guest and --elf")
    from dvt_circuits_amd import capi

    elf = guest_elf(args.guest) if args.guest else open(args.elf, "rb").read()
    stdin = [open(f, "rb").read() for f in args.stdin]
    at = parse_at(args.at)
    ranges = [parse_dump(d) for d in args.dump]
    if args.host:
        rc, rep, prof, err = capi.execute_profile(elf, stdin)
        if prof is None:
            raise SystemExit("execute failed: %s" % err)
        if err:
            print("the guest failed: %s" % err)

        def take(ranges):
            rc, _, snap, err = capi.execute_snapshot(elf, stdin, at, ranges, frames=args.frames, log_shard=args.log_shard)
            if snap is None:
                raise SystemExit("snapshot failed: %s" % err)
            return snap
        close = lambda: None
    else:
        p = capi.Prover('{"log_shard_size": %d}' % args.log_shard)
        pk, _ = p.setup(elf)
        job, rep = p.prepare(pk, stdin)
        prof = p.job_profile(pk, job, 0)
        take = lambda ranges: p.job_snapshot(pk, job, at, ranges, args.frames)

        def close():
            p.job_free(job)
            p.pk_free(pk)
            p.close()
    funcs, _ = flat_profile(elf, prof)
    spans = sorted((f["pc"], f["end"], f["name"]) for f in funcs)
    function_of = lambda pc: next((name for lo, hi, name in spans if lo <= pc < hi), spans[0][2] if spans and pc < spans[0][0] else "?")
    snap = take(ranges)
    if args.stack > 0:   # the second call: the stack pointer is a register of the first
        sp = snap["regs"][2]["value"]
        ranges = ranges + [capi.snap_range(sp, args.stack)]
        snap = take(ranges)
    for line in format_snapshot(snap, ranges, function_of):
        print(line)
    close()


if __name__ == "__main__":
    main()
