#!/usr/bin/env python3
"""What the memory report costs beside the flat execution report, on one GPU in one process.

    python tools/bench_memory.py [--shards 32] [--reps 3] [--out FILE.jsonl]

Per workload one JSON line: summary["ms"] of every repetition of Prover.job_memory and of Prover.job_profile on the same
prepared job (milliseconds inside the library after the entry guard, listed individually, the first call of each included),
and the report's totals.  Both calls read the same cycle records.  Workloads: the dkg_like guest that bench.py and
tools/bench_long_job.py build for --shards shards of 2^21 cycles, and tests/guests.bignum(40) (one short shard: the fixed
costs of a call, of which zeroing the 29.4 MB footprint bitmap is the largest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(prover, name, elf, stdin, reps):
    pk, _ = prover.setup(elf)
    job, rep = prover.prepare(pk, stdin)
    row = dict(workload=name, cycles=int(rep["cycles"]), shards=prover.job_shards(job), memory_ms=[], profile_ms=[])
    mem = None
    for _ in range(reps):
        mem = prover.job_memory(pk, job)
        row["memory_ms"].append(round(mem["summary"]["ms"], 3))
    for _ in range(reps):
        prof = prover.job_profile(pk, job)
        row["profile_ms"].append(round(prof["summary"]["ms"], 3))
    s = mem["summary"]
    assert s["cycles"] == prof["summary"]["cycles"] == rep["cycles"] and int(mem["first_touch"].sum()) == s["first_touches"]
    row.update({k: s[k] for k in ("loads", "stores", "pre_reads", "pre_writes", "pre_calls", "words", "first_touches", "n_pages", "mem_init_rows",
                                  "sp_writes")})
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
        row = measure(prover, name, elf, stdin, args.reps)
        print(json.dumps(row), flush=True)
        lines.append(row)
    prover.close()
    if args.out:
        with open(args.out, "w") as f:
            for row in lines:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
