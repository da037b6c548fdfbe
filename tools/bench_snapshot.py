#!/usr/bin/env python3
"""What a snapshot costs beside one pass of the memory report, on one GPU in one process.

    python tools/bench_snapshot.py [--shards 32] [--reps 3] [--out FILE.jsonl]

Per workload one JSON line: for three positions (in the first shard, in the middle of the execution, at the exit) and for 0,
64 and 4096 watched words, every repetition's summary["ms"] (milliseconds inside the library after the entry guard, downloads
and the host's part included) and the reduce, gather and backtrace launches as stream events time them
(Prover.job_snapshot_times), with the depth of the stack and how many cells carry no value; beside them summary["ms"] of
Prover.job_memory on the same prepared job in the same run, which reads the same cycle records once.
Workloads: the dkg_like guest that bench.py and tools/bench_long_job.py build for --shards shards of 2^21 cycles, and
tests/guests.bignum(40) (one short shard: the fixed costs of a call).  The watched words are taken from the job's own memory
report: 64 words at the stack pointer of the snapshot, and the four most accessed pages."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(capi, prover, name, elf, stdin, reps):
    pk, _ = prover.setup(elf)
    job, rep = prover.prepare(pk, stdin)
    mem = prover.job_memory(pk, job)
    n = prover.job_shards(job)
    pages = [pg["page"] for pg in sorted(mem["pages"], key=lambda pg: -(pg["loads"] + pg["stores"]))[:4]] or [0x400000]
    row = dict(workload=name, cycles=int(rep["cycles"]), shards=n, memory_ms=[], calls=[])
    end = prover.job_snapshot(pk, job, capi.SNAP_EXIT)["summary"]
    places = [("first shard", (1, min(1000, end["row"] if n == 1 else 1000))), ("middle", ((n + 1) // 2, (end["row"] if n == 1 else 1 << 21) // 2)),
              ("exit", capi.SNAP_EXIT)]
    for label, at in places:
        sp = prover.job_snapshot(pk, job, at)["regs"][2]["value"] & ~3
        sets = [("0 words", []), ("64 words", [(sp, sp + 256)] if sp and sp + 256 <= 0x38000000 else [(pages[0], pages[0] + 256)]),
                ("4096 words", [(pg, pg + 4096) for pg in (pages * 4)[:4]])]
        for words, ranges in sets:
            out = dict(at=label, words=words, ms=[], reduce_ms=[], gather_ms=[], backtrace_ms=[])
            for _ in range(reps):
                snap = prover.job_snapshot(pk, job, at, ranges)
                t = prover.job_snapshot_times()
                out["ms"].append(round(snap["summary"]["ms"], 3))
                for k in ("reduce_ms", "gather_ms", "backtrace_ms"):
                    out[k].append(round(t[k], 3))
            s = snap["summary"]
            assert s["cycles"] == rep["cycles"]
            out.update(position=s["position"], depth=s["depth"], n_words=s["n_words"], no_value=s["no_value"], untouched=s["untouched"])
            row["calls"].append(out)
    for _ in range(reps):
        row["memory_ms"].append(round(prover.job_memory(pk, job)["summary"]["ms"], 3))
    prover.job_free(job)
    prover.pk_free(pk)
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shards", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
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
        row = measure(capi, prover, name, elf, stdin, args.reps)
        print(json.dumps(row), flush=True)
        lines.append(row)
        if args.out:   # (written as it goes: a later workload that fails keeps the earlier line)
            with open(args.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")
    prover.close()


if __name__ == "__main__":
    main()
