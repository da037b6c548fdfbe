#!/usr/bin/env python3
"""What the call-tree report costs beside the flat execution report, on one GPU in one process.

    python tools/bench_calltree.py [--shards 32] [--reps 3] [--out FILE.jsonl]

Per workload one JSON line: the wall clock of every repetition of Prover.job_calltree and of Prover.job_profile on the same
prepared job (milliseconds, listed individually, the first call of each included), and the split of each job_calltree into
summary mode, the host's merge and emit mode (Prover.job_calltree_times).  Workloads: bench.py's default job (the
finalization-shaped guest fitted to --shards shards of 2^21 cycles), the finalization guest on the reference's example input,
and tests/guests_calltree.dense sized to two full shards, where nearly every record is an event and the single-lane walk of a
span is at its longest."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(prover, name, elf, stdin, reps):
    pk, _ = prover.setup(elf)
    job, rep = prover.prepare(pk, stdin)
    row = dict(workload=name, cycles=int(rep["cycles"]), shards=prover.job_shards(job), calltree_ms=[], calltree_split=[], profile_ms=[])
    tree = None
    for _ in range(reps):
        t = time.perf_counter()
        tree = prover.job_calltree(pk, job)
        row["calltree_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
        row["calltree_split"].append({k: round(v, 3) for k, v in prover.job_calltree_times().items()})
    for _ in range(reps):
        t = time.perf_counter()
        prof = prover.job_profile(pk, job)
        row["profile_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
    s = tree["summary"]
    assert s["cycles"] == prof["summary"]["cycles"] == rep["cycles"] and sum(f[3] for f in tree["funcs"]) == s["cycles"]
    row.update({k: s[k] for k in ("n_frames", "n_arcs", "n_funcs", "max_depth", "dropped_frames")})
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
    from tests import guests, guests_calltree, guests_finalization

    example = bench.workload_stdin(0)
    consts = bench.fit_constants(example, args.shards)
    work = [("bench.py default: dkg_like%r, %d shards" % (consts, args.shards), guests.dkg_like("finalization", *consts, **bench.guest_kw()), [example]),
            ("finalization guest (nmax = 8, kmax = 8) on the reference example", guests_finalization.finalization(nmax=8, kmax=8), [example]),
            ("guests_calltree.dense(16200): two shards of back-to-back calls", guests_calltree.dense(16200), [])]
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
