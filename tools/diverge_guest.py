#!/usr/bin/env python3
"""Where two runs of one guest part ways: the lock-step comparison of their cycle records (dvt_rv32_job_diverge on the GPU,
dvt_execute_diverge with --host; the rule is stated in csrc/diverge.h).

    python tools/diverge_guest.py --guest 'finalization_like(6, bytes(160))' --stdin-a A.bin --stdin-b B.bin [--host] [--rejoin N] [--origin]
    python tools/diverge_guest.py --elf guest.elf --stdin-a A.bin --stdin-b B.bin --from 1:0 --against-from 1:0 [--keep K] [--log-shard L]

One block per lock-step segment: how many pairs ran in step and why they stopped, the deciding pair (the last pair in step: the
branch or jalr whose operands differed) and the pair at the stop, the registers that hold different values at the stop, and the
first and last K data pairs.  With --rejoin N the comparison is repeated from the rejoin positions up to N times.  With --origin
the differing operand of the first deciding instruction is followed back in both runs (job_origin / execute_origin): the answer
reaches back to the hinted word or the syscall result that made the runs differ.  On the GPU both runs must prepare (exit 0
without a trap); --host also takes runs that trap or exit non-zero."""
import argparse
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.origin_guest import format_origin  # noqa: E402
from tools.profile_guest import guest_elf  # noqa: E402
from tools.snapshot_guest import ABI, parse_at  # noqa: E402

NONE, NO_REJOIN = 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF
REASONS = {1: "split", 2: "met a bad record", 3: "both runs ended", 4: "run A ended", 5: "run B ended", 6: "reached the pair limit"}
MASK = ((1, "rd"), (2, "rs1"), (4, "rs2"), (8, "mem"))


def word_at(elf, addr):
    """the word the ELF's image holds at addr, or None"""
    phoff, = struct.unpack_from("<I", elf, 28)
    phentsize, phnum = struct.unpack_from("<HH", elf, 42)
    for k in range(phnum):
        typ, off, vaddr, _, filesz = struct.unpack_from("<5I", elf, phoff + k * phentsize)
        if typ == 1 and vaddr <= addr and addr + 4 <= vaddr + filesz:
            return struct.unpack_from("<I", elf, off + addr - vaddr)[0]
    return None


def _rec(name, r):
    return "%s: none" % name if r is None else "%s: pc 0x%08x rd 0x%08x rs1 0x%08x rs2 0x%08x mem 0x%08x" % (name, r["pc"], r["a"], r["b"], r["c"], r["m_prev"])


def format_pair(part, e):
    text = "  %s %d  %d:%d / %d:%d pc 0x%08x differs in %s: rd 0x%08x / 0x%08x rs1 0x%08x / 0x%08x rs2 0x%08x / 0x%08x" % (
        part, e["k"], e["shard_a"], e["row_a"], e["shard_b"], e["row_b"], e["pc"], "+".join(n for bit, n in MASK if e["mask"] & bit), e["a_a"], e["a_b"], e["b_a"],
        e["b_b"], e["c_a"], e["c_b"])
    if e["dir"]:
        text += " %s [0x%08x] 0x%08x -> 0x%08x / [0x%08x] 0x%08x -> 0x%08x" % ("load" if e["dir"] == 1 else "store", e["addr_a"], e["before_a"], e["after_a"],
                                                                             e["addr_b"], e["before_b"], e["after_b"])
    return text


def format_report(got):
    """the lines of one block (capi's dict)"""
    s = got["summary"]
    lines = ["%d pairs in step, then %s at %d:%d / %d:%d (runs of %d and %d instructions); %d data pairs (%d loads, %d stores differ)" % (
        s["n_pairs"], REASONS.get(s["reason"], "?"), s["stop_shard_a"], s["stop_row_a"], s["stop_shard_b"], s["stop_row_b"], s["cycles_a"], s["cycles_b"], s["n_data"],
        s["n_load_diffs"], s["n_store_diffs"])]
    lines += [_rec("deciding A", s["prev_a"]), _rec("deciding B", s["prev_b"]), _rec("stop A", s["stop_a"]), _rec("stop B", s["stop_b"])]
    lines.append("live:" + "".join(" %s" % ABI[r] for r in range(1, 32) if got["regs"][r]["live"]))
    if s["rejoin_skip_a"] != NO_REJOIN:
        lines.append("rejoin at %d:%d (+%d) / %d:%d (+%d)" % (s["rejoin_shard_a"], s["rejoin_row_a"], s["rejoin_skip_a"], s["rejoin_shard_b"], s["rejoin_row_b"],
                                                             s["rejoin_skip_b"]))
    lines += [format_pair("first", e) for e in got["first"]] + [format_pair("last", e) for e in got["last"]]
    return lines


def deciding_origins(got, origin, stdin_a, stdin_b, elf):
    """The differing operand of the deciding instruction of a report, followed back in both runs: ((what, register), [slice of A,
    slice of B]) or (None, []) when the report has no deciding pair whose operands differ.  origin(stdin, at, target) -> slice."""
    s = got["summary"]
    a, b = s["prev_a"], s["prev_b"]
    if a is None or b is None or (a["b"] == b["b"] and a["c"] == b["c"]):
        return None, []
    word = word_at(elf, a["pc"])
    if word is None:
        return None, []
    reg = (word >> 15) & 31 if a["b"] != b["b"] else (word >> 20) & 31
    if not reg:
        return None, []
    target = (1, reg)
    starts = ((s["stop_shard_a"], s["stop_row_a"]), (s["stop_shard_b"], s["stop_row_b"]))
    # the deciding record is the one before the stop: ask before it; at row 0 it ends the shard before, and the question is asked
    # at the stop itself (a branch writes no register, so the operand is still what it read)
    slices = []
    for stdin, (shard, row) in zip((stdin_a, stdin_b), starts):
        at = (shard, row - 1) if row else (shard, row)
        slices.append(origin(stdin, at, target))
    return target, slices


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--guest")
    ap.add_argument("--elf")
    ap.add_argument("--stdin-a", required=True)
    ap.add_argument("--stdin-b", required=True)
    ap.add_argument("--from", dest="start_a", default="1:0", metavar="S:R")
    ap.add_argument("--against-from", dest="start_b", default="1:0", metavar="S:R")
    ap.add_argument("--rejoin", type=int, default=0, metavar="N")
    ap.add_argument("--keep", type=int, default=4)
    ap.add_argument("--origin", action="store_true", help="follow the differing operand of the deciding instruction back in both runs")
    ap.add_argument("--host", action="store_true", help="on the host (dvt_execute_diverge): no GPU is touched")
    ap.add_argument("--log-shard", type=int, default=21)
    args = ap.parse_args()
    if bool(args.guest) == bool(args.elf):
        ap.error("one of --guest and --elf")
    try:
        at_a, at_b = parse_at(args.start_a), parse_at(args.start_b)
    except ValueError as e:
        ap.error(str(e))
    from dvt_circuits_amd import capi

    elf = guest_elf(args.guest) if args.guest else open(args.elf, "rb").read()
    a, b = open(args.stdin_a, "rb").read(), open(args.stdin_b, "rb").read()
    p = pk = None
    if args.host:
        def call(**kw):
            rc, reps, got, err = capi.execute_diverge(elf, a, b, log_shard=args.log_shard, keep=args.keep, **kw)
            if got is None:
                raise SystemExit("diverge failed: %s" % err)
            return got
        origin = lambda stdin, at, target: capi.execute_origin(elf, [stdin], at, target, log_shard=args.log_shard)[2]
    else:
        p = capi.Prover('{"log_shard_size": %d}' % args.log_shard)
        pk, _ = p.setup(elf)
        jobs = {a: p.prepare(pk, [a])[0]}
        jobs[b] = jobs[a] if b == a else p.prepare(pk, [b])[0]
        call = lambda **kw: p.job_diverge(pk, jobs[a], jobs[b], keep=args.keep, **kw)
        origin = lambda stdin, at, target: p.job_origin(pk, jobs[stdin], at, target)
    first = None
    for k in range(args.rejoin + 1):
        got = call(start_a=at_a, start_b=at_b, rejoin=True)
        first = first or got
        if p:
            print("classify %.3f ms, merge %.3f ms, emit %.3f ms, host %.3f ms" % tuple(p.job_diverge_times()[x] for x in ("classify_ms", "merge_ms", "emit_ms", "host_ms")))
        for line in format_report(got):
            print(line)
        s = got["summary"]
        if s["reason"] != 1 or s["rejoin_skip_a"] == NO_REJOIN:
            break
        at_a, at_b = (s["rejoin_shard_a"], s["rejoin_row_a"]), (s["rejoin_shard_b"], s["rejoin_row_b"])
    if args.origin:
        target, slices = deciding_origins(first, origin, a, b, elf)
        if target is None:
            print("no deciding operand differs")
        for name, sl in zip("AB", slices):
            print("origin of %s in run %s:" % (ABI[target[1]], name))
            for line in format_origin(sl, target[0]):
                print("  " + line)
    if p:
        for job in set(jobs.values()):
            p.job_free(job)
        p.pk_free(pk)
        p.close()


if __name__ == "__main__":
    main()
