#!/usr/bin/env python3
"""Where a guest's cycles go: a flat profile from the execution report (dvt_rv32_job_profile on the GPU, dvt_execute_profile
with --host).

    python tools/profile_guest.py --guest 'bignum(40)' [--top N] [--json OUT] [--host] [--log-shard L]
    python tools/profile_guest.py --elf guest.elf [--stdin FILE ...]
    python tools/profile_guest.py --guest 'bignum(40)' --calls [--host]
    python tools/profile_guest.py --guest 'bignum(40)' --memory [--host]

The guest is an expression over the functions of tests/guests*.py (its ELF is the value, or the first element of it), or an
ELF file with its stdin buffers.  The guests are stripped (tools/rvasm.py writes program headers only), so function entries
come from the report itself: the ELF entry plus the target of every edge whose source is a `jal` / `jalr` that writes ra.
Every instruction belongs to the nearest entry at or below it.  Prints per function f_<pc> its cycles, its share and its
calls (the counts of the edges into the entry), then the hottest taken branches, the opcode and the syscall counts; --json
writes the same with the raw tables.

--calls adds the call-tree report (dvt_rv32_job_calltree on the GPU, dvt_execute_calltree with --host): per function f_<pc> its
inclusive cycles, its self cycles and its calls, measured from the calls and returns of the execution instead of address ranges
(a tail jump or a shared helper is charged to the function that was called), then the heaviest caller -> callee arcs; --json
carries both tables.

--memory adds the memory report (dvt_rv32_job_memory on the GPU, dvt_execute_memory with --host): the accessed address ranges
(runs of consecutive pages merged) with their loads, stores, precompile reads and writes and distinct words; per function the
words its instructions touched first (first_touch summed over the same address ranges as the flat profile: every such word is
a row of the mem_init table), the remainder that precompile calls touched first, and the span of the stack pointer."""
import argparse
import importlib
import json
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def guest_elf(expr):
    scope = {}
    for mod in ("guests", "guests_bls", "guests_finalization", "guests_share", "guests_profile", "guests_calltree", "guests_memory"):
        m = importlib.import_module("tests." + mod)
        scope.update({k: getattr(m, k) for k in dir(m) if not k.startswith("_") and k not in scope})
    v = eval(expr if "(" in expr else expr + "()", scope)   # noqa: S307 (the caller's own command line)
    return v if isinstance(v, (bytes, bytearray)) else v[0]


def text_words(elf):
    """(text_base, raw words) of the executable segment"""
    phoff, = struct.unpack_from("<I", elf, 28)
    phentsize, phnum = struct.unpack_from("<HH", elf, 42)
    for k in range(phnum):
        typ, off, vaddr, _, filesz, _, flags, _ = struct.unpack_from("<8I", elf, phoff + k * phentsize)
        if typ == 1 and flags & 1:
            blob = elf[off:off + filesz] + b"\0" * (-filesz % 4)
            return vaddr, [w for (w,) in struct.iter_unpack("<I", blob)]
    raise SystemExit("no executable segment")


def links_ra(word):
    """a jal / jalr that writes ra (x1): a call"""
    return word & 0x7F in (0x6F, 0x67) and (word >> 7) & 31 == 1


def flat_profile(elf, prof):
    """functions = [dict(name, pc, end, cycles, share, calls)] by cycles descending; branches = the taken edges that are no
    calls and no returns, by count descending"""
    base, words = text_words(elf)
    entry, = struct.unpack_from("<I", elf, 24)
    word_at = lambda pc: words[(pc - base) // 4]
    calls = {}
    for a, b, c in prof["edges"]:
        if links_ra(word_at(a)):
            calls[b] = calls.get(b, 0) + c
    entries = sorted(set(calls) | {entry})
    pc_count, total = prof["pc_count"], max(int(prof["summary"]["cycles"]), 1)
    funcs = []
    for k, pc in enumerate(entries):
        end = entries[k + 1] if k + 1 < len(entries) else base + 4 * len(words)
        first = base if k == 0 else pc        # (what lies below the lowest entry goes to it)
        cyc = int(pc_count[(first - base) // 4:(end - base) // 4].sum())
        funcs.append(dict(name="f_%x" % pc, pc=pc, end=end, cycles=cyc, share=cyc / total, calls=calls.get(pc, 0)))
    funcs.sort(key=lambda f: (-f["cycles"], f["pc"]))
    is_ret = lambda w: w & 0x7F == 0x67 and (w >> 7) & 31 == 0
    branches = sorted(((c, a, b) for a, b, c in prof["edges"] if not links_ra(word_at(a)) and not is_ret(word_at(a))), reverse=True)
    return funcs, [dict(from_pc=a, to_pc=b, count=c) for c, a, b in branches]


def page_ranges(pages, page_bytes=4096):
    """runs of consecutive pages merged: [dict(first, last (inclusive byte addresses), loads, stores, pre_reads, pre_writes, words)]"""
    keys = ("loads", "stores", "pre_reads", "pre_writes", "words")
    out = []
    for pg in pages:
        if out and out[-1]["last"] + 1 == pg["page"]:
            out[-1]["last"] = pg["page"] + page_bytes - 1
            for k in keys:
                out[-1][k] += pg[k]
        else:
            out.append(dict({k: pg[k] for k in keys}, first=pg["page"], last=pg["page"] + page_bytes - 1))
    return out


def first_touch_by_function(elf, funcs, first_touch):
    """[dict(name, pc, words)] by words descending: first_touch summed over the address range of every function of flat_profile"""
    base, _ = text_words(elf)
    lowest = min(f["pc"] for f in funcs)
    rows = [dict(name=f["name"], pc=f["pc"], words=int(first_touch[((base if f["pc"] == lowest else f["pc"]) - base) // 4:(f["end"] - base) // 4].sum()))
            for f in funcs]
    return sorted((r for r in rows if r["words"]), key=lambda r: (-r["words"], r["pc"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--guest")
    ap.add_argument("--elf")
    ap.add_argument("--stdin", action="append", default=[])
    ap.add_argument("--top", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--host", action="store_true", help="tally on the host (dvt_execute_profile): no GPU is touched")
    ap.add_argument("--log-shard", type=int, default=21)
    ap.add_argument("--log-edge-slots", type=int, default=0)
    ap.add_argument("--calls", action="store_true", help="also the call-tree report: inclusive and self cycles per function, the heaviest arcs")
    ap.add_argument("--log-arc-slots", type=int, default=0)
    ap.add_argument("--memory", action="store_true", help="also the memory report: accessed ranges, first touches per function, the stack span")
    args = ap.parse_args()
    if bool(args.guest) == bool(args.elf):
        ap.error("one of --guest and --elf")
    from dvt_circuits_amd import capi

    elf = guest_elf(args.guest) if args.guest else open(args.elf, "rb").read()
    stdin = [open(f, "rb").read() for f in args.stdin]
    if args.host:
        rc, rep, prof, err = capi.execute_profile(elf, stdin)
        if prof is None:
            raise SystemExit("execute failed: %s" % err)
        tree = capi.execute_calltree(elf, stdin)[2] if args.calls else None
        mem = capi.execute_memory(elf, stdin)[2] if args.memory else None
        if rc:
            print("the guest failed (%s): the profile of what retired" % err)
    else:
        p = capi.Prover('{"log_shard_size": %d}' % args.log_shard)
        pk, _ = p.setup(elf)
        job, rep = p.prepare(pk, stdin)
        prof = p.job_profile(pk, job, args.log_edge_slots)
        tree = p.job_calltree(pk, job, args.log_arc_slots) if args.calls else None
        mem = p.job_memory(pk, job) if args.memory else None
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    s = prof["summary"]
    funcs, branches = flat_profile(elf, prof)
    print("%d cycles, %d instructions in the text, %d transfers over %d edges (%d dropped), %d of %d shards, %.2f ms" %
          (s["cycles"], s["n_instr"], s["n_transfers"], s["n_edges"], s["dropped_transfers"], s["shards_tallied"], s["shards_total"], s["ms"]))
    print("%-12s %14s %7s %12s" % ("function", "cycles", "share", "calls"))
    for f in funcs[:args.top]:
        print("%-12s %14d %6.2f%% %12d" % (f["name"], f["cycles"], 100 * f["share"], f["calls"]))
    print("hottest taken branches:")
    for b in branches[:args.top]:
        print("  0x%08x -> 0x%08x %14d" % (b["from_pc"], b["to_pc"], b["count"]))
    print("opcodes: " + ", ".join("%s %d" % kv for kv in sorted(prof["opcodes"].items(), key=lambda kv: (-kv[1], kv[0]))[:args.top]))
    print("syscalls: " + ", ".join("0x%x %d" % kv for kv in sorted(prof["syscalls"].items())))
    calls = {}
    if tree:
        t = tree["summary"]
        total = max(t["cycles"], 1)
        print("call tree: %d frames over %d arcs (%d frames, %d cycles dropped), depth %d, %d open at the exit, %d unmatched returns, %.2f ms" %
              (t["n_frames"], t["n_arcs"], t["dropped_frames"], t["dropped_cycles"], t["max_depth"], t["open_at_exit"], t["unmatched_returns"], t["ms"]))
        print("%-12s %14s %14s %7s %12s" % ("function", "inclusive", "self", "share", "calls"))
        for pc, n, inc, own in tree["funcs"][:args.top]:
            print("%-12s %14d %14d %6.2f%% %12d" % ("f_%x" % pc, inc, own, 100 * own / total, n))
        print("heaviest arcs:")
        for caller, callee, n, cyc in sorted(tree["arcs"], key=lambda a: -a[3])[:args.top]:
            print("  %-12s -> %-12s %14d cycles %12d calls" % ("(root)" if caller is None else "f_%x" % caller, "f_%x" % callee, cyc, n))
        calls = dict(calltree=dict(summary=t, functions=[dict(name="f_%x" % pc, pc=pc, calls=n, inclusive=inc, self=own) for pc, n, inc, own in tree["funcs"]],
                                   arcs=[dict(caller_pc=a, callee_pc=b, calls=n, cycles=c) for a, b, n, c in tree["arcs"]]))
    if mem:
        m = mem["summary"]
        ranges, by_func = page_ranges(mem["pages"], m["page_bytes"]), first_touch_by_function(elf, funcs, mem["first_touch"])
        print("memory: %d words on %d pages (%d of the %d image words), mem_init rows %d; %d loads, %d stores, %d precompile calls with %d reads and %d writes, "
              "%d of %d shards, %.2f ms" % (m["words"], m["n_pages"], m["image_words_accessed"], m["image_words"], m["mem_init_rows"], m["loads"], m["stores"],
                                            m["pre_calls"], m["pre_reads"], m["pre_writes"], m["shards_tallied"], m["shards_total"], m["ms"]))
        print("%-23s %12s %12s %12s %12s %10s" % ("range", "loads", "stores", "pre reads", "pre writes", "words"))
        for r in ranges:
            print("0x%08x-0x%08x %12d %12d %12d %12d %10d" % (r["first"], r["last"], r["loads"], r["stores"], r["pre_reads"], r["pre_writes"], r["words"]))
        print("%-12s %14s   (words first touched by a load or store of the function)" % ("function", "first touches"))
        for f in by_func[:args.top]:
            print("%-12s %14d" % (f["name"], f["words"]))
        print("first touched by precompile calls (or outside the held shards): %d words" % (m["words"] - m["first_touches"]))
        print("stack pointer: %d writes, 0x%08x .. 0x%08x (%d bytes)" % (m["sp_writes"], m["sp_min"], m["sp_max"], m["sp_max"] - m["sp_min"]))
        calls = dict(calls, memory=dict(summary=m, ranges=ranges, pages=mem["pages"], first_touch=[int(x) for x in mem["first_touch"]],
                                        first_touch_by_function=by_func, precompile_first_touches=m["words"] - m["first_touches"],
                                        stack=dict(writes=m["sp_writes"], min=m["sp_min"], max=m["sp_max"])))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(calls, summary=s, functions=funcs, branches=branches, opcodes=prof["opcodes"], syscalls={"0x%x" % k: v for k, v in prof["syscalls"].items()},
                           pc_count=[int(x) for x in prof["pc_count"]], edges=prof["edges"]), f, indent=1)


if __name__ == "__main__":
    main()
