#!/usr/bin/env python3
"""Watchpoints on a guest: which instruction ran a pc, wrote a register or accessed a word, with what values and in what order
(dvt_rv32_job_watch on the GPU, dvt_execute_watch with --host; the rule is stated in csrc/watch.h).

    python tools/watch_guest.py --guest 'hammer()' --watch store:0x3000f8 --watch reg:sp=0xf0/0xff0 [--keep K] [--host]
    python tools/watch_guest.py --guest 'bignum(40)' --watch pc:0x2008a0 --from 3:100 --to 5:0 [--log-shard L]
    python tools/watch_guest.py --elf guest.elf [--stdin FILE ...] --history 0x3000f8

A --watch spec (repeatable, at most 16):
    pc:ADDR[+BYTES]                     the instructions at ADDR .. ADDR + BYTES (default 4)
    reg:NAME[=VALUE[/MASK]]             writes of a register (x1..x31 or an ABI name), optionally of (VALUE & MASK)
    load: store: pread: pwrite: mem:    ADDR[+BYTES][=VALUE[/MASK]]  accesses of the words in ADDR .. ADDR + BYTES (default 4): loads,
                                        stores, precompile reads, precompile writes, all four; =VALUE: the loads and stores that
                                        leave (VALUE & MASK) in the word
--from S:R / --to S:R restrict every spec to the positions from <= (shard, row) < to; shards are numbered from 1, row is the
index of the instruction in its shard.  Per spec the tool prints the exact number of hits and the first and the last --keep of
them, one line per hit with the function it belongs to, found the way tools/profile_guest.py finds functions.

--history ADDR follows the previous-access pointer of the hits backwards from the last access of the word at ADDR and prints
every load and store of it, newest first, and where the chain stops: at the first touch of the word, or at an access that no
load or store made (a precompile call, whose record does not carry the pointer)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.profile_guest import flat_profile, guest_elf  # noqa: E402

PC, REG, MEM = 1, 2, 3
LOAD, STORE, PRE_READ, PRE_WRITE, VALUE, NO_VALUE = 1, 2, 4, 8, 16, 32
ABI = ["zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1"] + ["a%d" % i for i in range(8)] + ["s%d" % i for i in range(2, 12)] + \
      ["t3", "t4", "t5", "t6"]
MEM_KINDS = {"load": LOAD, "store": STORE, "pread": PRE_READ, "pwrite": PRE_WRITE, "mem": LOAD | STORE | PRE_READ | PRE_WRITE}
EVERYWHERE = ((0, 0), (0xFFFFFFFF, 0xFFFFFFFF))


def _value(text):
    """=VALUE[/MASK] split off: (rest, value or None, mask)"""
    if "=" not in text:
        return text, None, 0
    text, v = text.split("=", 1)
    v, m = v.split("/", 1) if "/" in v else (v, "0xffffffff")
    return text, int(v, 0), int(m, 0)


def _range(text):
    a, n = text.split("+", 1) if "+" in text else (text, "4")
    return int(a, 0), int(a, 0) + int(n, 0)


def parse_spec(spec, window=EVERYWHERE):
    """a --watch spec as the query dict of dvt_circuits_amd.capi (watch_pc / watch_reg / watch_mem give the same)"""
    kind, _, rest = spec.partition(":")
    (fs, fr), (ts, tr) = window
    q = dict(kind=0, flags=0, lo=0, hi=0, mask=0, want=0, from_shard=fs, from_row=fr, to_shard=ts, to_row=tr)
    if kind == "pc":
        lo, hi = _range(rest)
        q.update(kind=PC, lo=lo, hi=hi)
    elif kind == "reg":
        name, want, mask = _value(rest)
        reg = ABI.index(name) if name in ABI else int(name[1:]) if name[:1] == "x" and name[1:].isdigit() else -1
        if not 1 <= reg <= 31:
            raise ValueError("no register that can be watched: %r" % name)
        q.update(kind=REG, lo=reg, hi=reg + 1, flags=0 if want is None else VALUE, want=want or 0, mask=mask)
    elif kind in MEM_KINDS:
        rest, want, mask = _value(rest)
        lo, hi = _range(rest)
        q.update(kind=MEM, lo=lo & ~3, hi=(hi + 3) & ~3, flags=MEM_KINDS[kind] | (0 if want is None else VALUE), want=want or 0, mask=mask)
    else:
        raise ValueError("unknown watch spec %r (pc: reg: load: store: pread: pwrite: mem:)" % spec)
    return q


def format_spec(q):
    """the spec of a query dict (without its window): parse_spec(format_spec(q)) == q for every q that parse_spec can give"""
    value = "=0x%x/0x%x" % (q["want"], q["mask"]) if q["flags"] & VALUE else ""
    if q["kind"] == PC:
        return "pc:0x%x+%d" % (q["lo"], q["hi"] - q["lo"])
    if q["kind"] == REG:
        return "reg:%s%s" % (ABI[q["lo"]], value)
    names = {v: k for k, v in MEM_KINDS.items()}
    return "%s:0x%x+%d%s" % (names[q["flags"] & ~VALUE], q["lo"], q["hi"] - q["lo"], value)


def parse_position(text):
    s, _, r = text.partition(":")
    return int(s, 0), int(r or "0", 0)


def format_hit(h, function_of=lambda pc: ""):
    what = ""
    if h["flags"] & (LOAD | STORE):
        what = " %s 0x%08x: 0x%08x -> 0x%08x, before it (%d, clk %d)" % ("load " if h["flags"] & LOAD else "store", h["addr"], h["before"], h["after"],
                                                                        h["prev_shard"], h["prev_clk"])
    elif h["flags"] & NO_VALUE:
        what = " call%s%s of %d words from 0x%08x" % (" reads" if h["flags"] & PRE_READ else "", " writes" if h["flags"] & PRE_WRITE else "", h["n_words"],
                                                      h["addr"])
    return "  %5d:%-8d pc 0x%08x %-10s rd 0x%08x rs1 0x%08x rs2 0x%08x%s" % (h["shard"], h["row"], h["pc"], function_of(h["pc"]), h["rd_value"], h["rs1"],
                                                                              h["rs2"], what)


def history(search, addr, batch=256):
    """The loads and stores of the word at addr, newest first, by following (prev_shard, prev_clk) from the last one.
    search(queries, keep) -> per query dict(total, first, last).  Returns (hits, why the chain stopped)."""
    addr &= ~3
    out, to = [], EVERYWHERE[1]
    want = None                              # the position the chain points at; None: the last access there is
    while True:
        q = dict(kind=MEM, flags=LOAD | STORE, lo=addr, hi=addr + 4, mask=0, want=0, from_shard=0, from_row=0, to_shard=to[0], to_row=to[1])
        found = search([q], batch)[0]
        by_pos = {(h["shard"], h["row"]): h for h in found["last"]}
        if want is None:
            if not found["last"]:
                return out, "no load or store accesses the word"
            want = (found["last"][-1]["shard"], found["last"][-1]["row"])
        while want in by_pos:
            h = by_pos[want]
            out.append(h)
            if (h["prev_shard"], h["prev_clk"]) == (0, 0):
                return out, "first touch of the word"
            # the memory port of row r works at clk 4 r + 6; a precompile call touches its words at 4 r + 6 or 4 r + 7
            want = (h["prev_shard"], h["prev_clk"] // 4 - 1)
        if want not in by_pos and (to == (want[0], want[1] + 1) or not found["last"]):
            return out, "the access before, at %d:%d, is no load or store (a precompile call or a shard that is not held)" % want
        to = (want[0], want[1] + 1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--guest")
    ap.add_argument("--elf")
    ap.add_argument("--stdin", action="append", default=[])
    ap.add_argument("--watch", action="append", default=[], metavar="SPEC")
    ap.add_argument("--from", dest="from_", default="0:0", metavar="S:R")
    ap.add_argument("--to", default="0xffffffff:0xffffffff", metavar="S:R")
    ap.add_argument("--keep", type=int, default=8)
    ap.add_argument("--history", metavar="ADDR")
    ap.add_argument("--host", action="store_true", help="search on the host (dvt_execute_watch): no GPU is touched")
    ap.add_argument("--log-shard", type=int, default=21)
    args = ap.parse_args()
    if bool(args.guest) == bool(args.elf):
        ap.error("one of --guest and --elf")
    if not args.watch and not args.history:
        ap.error("nothing to watch: --watch SPEC or --history ADDR")
    from dvt_circuits_amd import capi

    elf = guest_elf(args.guest) if args.guest else open(args.elf, "rb").read()
    stdin = [open(f, "rb").read() for f in args.stdin]
    window = (parse_position(args.from_), parse_position(args.to))
    queries = [parse_spec(s, window) for s in args.watch]
    if args.host:
        rc, rep, prof, err = capi.execute_profile(elf, stdin)
        if prof is None:
            raise SystemExit("execute failed: %s" % err)

        def search(qs, keep):
            rc, _, found, err = capi.execute_watch(elf, stdin, qs, keep=keep, log_shard=args.log_shard)
            if found is None:
                raise SystemExit("watch failed: %s" % err)
            return found
        close = lambda: None
    else:
        p = capi.Prover('{"log_shard_size": %d}' % args.log_shard)
        pk, _ = p.setup(elf)
        job, rep = p.prepare(pk, stdin)
        prof = p.job_profile(pk, job, 0)
        search = lambda qs, keep: p.job_watch(pk, job, qs, keep=keep)

        def close():
            p.job_free(job)
            p.pk_free(pk)
            p.close()
    funcs, _ = flat_profile(elf, prof)
    spans = sorted((f["pc"], f["end"], f["name"]) for f in funcs)
    function_of = lambda pc: next((name for lo, hi, name in spans if lo <= pc < hi), spans[0][2] if spans and pc < spans[0][0] else "?")
    if queries:
        for spec, found in zip(args.watch, search(queries, args.keep)):
            k = len(found["first"])
            print("%s: %d hits" % (spec, found["total"]))
            for h in found["first"]:
                print(format_hit(h, function_of))
            if found["total"] > k:
                skipped = found["total"] - 2 * k
                if skipped > 0:
                    print("  ... %d more ..." % skipped)
                for h in found["last"][max(0, 2 * k - found["total"]):]:
                    print(format_hit(h, function_of))
    if args.history:
        hits, why = history(search, int(args.history, 0))
        print("history of 0x%08x: %d loads and stores, newest first" % (int(args.history, 0) & ~3, len(hits)))
        for h in hits:
            print(format_hit(h, function_of))
        print("  the chain stops: %s" % why)
    close()


if __name__ == "__main__":
    main()
