#!/usr/bin/env python3
"""What a watchpoint search costs beside one pass of the memory report, on one GPU in one process.

    python tools/bench_watch.py [--shards 32] [--reps 3] [--keep 256] [--out FILE.jsonl]

Per workload one JSON line: for a call with 16 queries and for a call with one, every repetition's summary["ms"] (milliseconds
inside the library after the entry guard, downloads and the host's part included) and the count, scan and emit launches as
stream events time them (Prover.job_watch_times), the totals found, and the shards the emit pass ran over; beside them
summary["ms"] of Prover.job_memory on the same prepared job in the same run, which reads the same cycle records once.
Workloads: the dkg_like guest that bench.py and tools/bench_long_job.py build for --shards shards of 2^21 cycles, and
tests/guests.bignum(40) (one short shard: the fixed costs of a call).  The queries are made from the job's own reports: the
four hottest instructions, writes of sp, ra, a0 and (with a value filter) t0, and eight memory queries over the accessed
pages in every direction, with and without a value filter; the one-query call asks for the hottest instruction."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def queries_of(capi, prof, mem):
    tb = prof["summary"]["text_base"]
    hot = [tb + 4 * int(i) for i in prof["pc_count"].argsort()[::-1][:4]]
    pages = [pg["page"] for pg in sorted(mem["pages"], key=lambda pg: -(pg["loads"] + pg["stores"]))[:3]] or [0x400000]
    everything = (0, 0x38000000)
    pre = capi.DVT_WATCH_PRE_READ | capi.DVT_WATCH_PRE_WRITE
    qs = [capi.watch_pc(pc) for pc in hot]
    qs += [capi.watch_reg(2), capi.watch_reg(1), capi.watch_reg(10), capi.watch_reg(5, value=0x10)]
    qs += [capi.watch_mem(pages[0], pages[0] + 4096, flags=capi.DVT_WATCH_STORE), capi.watch_mem(pages[0], pages[0] + 4096, flags=capi.DVT_WATCH_LOAD),
           capi.watch_mem(pages[-1], pages[-1] + 64), capi.watch_mem(*everything, flags=pre), capi.watch_mem(*everything, flags=capi.DVT_WATCH_STORE, value=0),
           capi.watch_mem(*everything, flags=capi.DVT_WATCH_STORE, value=0xFF, mask=0xFF), capi.watch_mem(pages[0] + 128, pages[0] + 132),
           capi.watch_mem(*everything)]
    assert len(qs) == capi.DVT_WATCH_MAX_QUERIES
    return qs


def measure(capi, prover, name, elf, stdin, reps, keep):
    pk, _ = prover.setup(elf)
    job, rep = prover.prepare(pk, stdin)
    prof, mem = prover.job_profile(pk, job), prover.job_memory(pk, job)
    queries = queries_of(capi, prof, mem)
    row = dict(workload=name, cycles=int(rep["cycles"]), shards=prover.job_shards(job), keep=keep, memory_ms=[])
    for label, qs in (("sixteen", queries), ("one", queries[:1])):
        out = dict(ms=[], count_ms=[], scan_ms=[], emit_ms=[])
        for _ in range(reps):
            found, s = prover.job_watch(pk, job, qs, keep=keep, summary=True)
            t = prover.job_watch_times()
            out["ms"].append(round(s["ms"], 3))
            for k in ("count_ms", "scan_ms", "emit_ms"):
                out[k].append(round(t[k], 3))
            out["emit_shards"] = t["emit_shards"]
        assert s["cycles"] == rep["cycles"]
        out["totals"] = [f["total"] for f in found]
        row[label] = out
    for _ in range(reps):
        row["memory_ms"].append(round(prover.job_memory(pk, job)["summary"]["ms"], 3))
    prover.job_free(job)
    prover.pk_free(pk)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shards", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--keep", type=int, default=256)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    example = bench.workload_stdin()
    consts = bench.fit_constants(example, args.shards)
    work = [("dkg_like%r, %d shards" % (consts, args.shards), guests.dkg_like("finalization", *consts, **bench.guest_kw()), [example]),
            ("bignum(40)", guests.bignum(40)[0], [])]
    prover = capi.Prover('{"device": 0, "fri_queries": 100, "pow_bits": 16, "log_shard_size": 21}')
    lines = []
    for name, elf, stdin in work:
        row = measure(capi, prover, name, elf, stdin, args.reps, args.keep)
        print(json.dumps(row), flush=True)
        lines.append(row)
        if args.out:   # (written as it goes: a later workload that fails keeps the earlier line)
            with open(args.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")
    prover.close()


if __name__ == "__main__":
    main()
