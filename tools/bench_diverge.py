#!/usr/bin/env python3
"""What a divergence report costs beside the memory report, on one GPU in one process.

    python tools/bench_diverge.py [--shards 32] [--reps 5] [--lib LIBRARY.so] [--out FILE.jsonl]

Two jobs of the dkg_like guest that bench.py builds for --shards shards of 2^21 cycles are prepared in one handle (if the second
does not fit in HBM the shard count is halved until it does; the line says which count ran).  One JSON line with, per case, every
repetition's summary["ms"] after a dropped first call, its median, and the classify / merge / emit launches as stream events time
them (Prover.job_diverge_times):
    identical     the two jobs of the same input from the entry: the whole prefix is read, the worst case
    one_byte      against the job of the input with byte 8 changed (the runs split after some ten thousand pairs)
    early_split   job A from its entry against job B from its second record: out of step at once, so the first batch holds the stop
    memory        Prover.job_memory on job A, which reads one record stream once
--lib loads another build of the library, for instance one compiled with -DDVT_DIVERGE_BATCH_PAIRS=...; launched_pairs of
early_split is the batch size it ran with."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(reps, call, times=None):
    """every repetition after a dropped first call: (summary of the last, [ms], {stage: [ms]})"""
    call()
    ms, stages = [], {}
    for _ in range(reps):
        s = call()
        ms.append(round(s["ms"], 3))
        for k, v in (times() if times else {}).items():
            stages.setdefault(k, []).append(round(v, 3))
    return s, ms, stages


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shards", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lib")
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    if args.lib:
        capi.LIB_PATH = os.path.abspath(args.lib)
    example = bench.workload_stdin()
    changed = bytearray(example)
    changed[8] ^= 1   # (the first byte behind the buffer's length: the guest folds it into what it hashes)
    shards = args.shards
    while True:
        consts = bench.fit_constants(example, shards)
        elf = guests.dkg_like("finalization", *consts, **bench.guest_kw())
        prover = capi.Prover('{"device": 0, "fri_queries": 100, "pow_bits": 16, "log_shard_size": 21}')
        pk, _ = prover.setup(elf)
        try:
            jobs = [prover.prepare(pk, [buf])[0] for buf in (example, example, bytes(changed))]
            break
        except capi.DvtError as e:
            print("%d shards: %s" % (shards, e), file=sys.stderr)
            prover.close()
            shards //= 2
            if not shards:
                raise
    row = dict(workload="dkg_like%r" % (consts,), shards_asked=args.shards, shards=prover.job_shards(jobs[0]), lib=args.lib or "default", cases={})
    cases = [("identical", jobs[0], jobs[1], {}), ("one_byte", jobs[0], jobs[2], {}), ("early_split", jobs[0], jobs[1], dict(start_b=(1, 1)))]
    for name, a, b, kw in cases:
        s, ms, stages = timed(args.reps, lambda: prover.job_diverge(pk, a, b, rejoin=True, keep=16, **kw)["summary"], prover.job_diverge_times)
        row["cases"][name] = dict(ms=ms, median_ms=statistics.median(ms), spread_ms=round(max(ms) - min(ms), 3), **stages,
                                  **{k: s[k] for k in ("n_pairs", "reason", "n_data", "launched_pairs", "cycles_a", "cycles_b", "rejoin_skip_a", "rejoin_skip_b")})
    s, ms, _ = timed(args.reps, lambda: prover.job_memory(pk, jobs[0])["summary"])
    row["cases"]["memory"] = dict(ms=ms, median_ms=statistics.median(ms), spread_ms=round(max(ms) - min(ms), 3), cycles=s["cycles"])
    print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
    for job in jobs:
        prover.job_free(job)
    prover.pk_free(pk)
    prover.close()


if __name__ == "__main__":
    main()
