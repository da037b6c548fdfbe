#!/usr/bin/env python3
"""What an origin slice costs beside the snapshot's reduce pass, on one GPU in one process.

    python tools/bench_origin.py [--shards 32] [--reps 3] [--out FILE.jsonl]

Per workload one JSON line: a0, and the register whose slice from the exit takes the most passes (found by asking all 31), at
the exit and in the middle of the execution, with depth 8 and 64 (1024 nodes, 8192 edges), every repetition's summary["ms"] (milliseconds inside the library after the entry guard, uploads, downloads and the host's
search included) and the reduce and gather launches as stream events time them, summed over the levels and passes of the call
(Prover.job_origin_times), with the number of passes, so that reduce_ms / passes is one pass over the records before the
positions asked at; beside them the reduce pass of Prover.job_snapshot without words at the same position in the same run,
which reads the records of every shard once.
Workloads: the dkg_like guest that bench.py and tools/bench_long_job.py build for --shards shards of 2^21 cycles, and
tests/guests.bignum(40) (one short shard: the fixed costs of a call)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(capi, prover, name, elf, stdin, reps):
    pk, _ = prover.setup(elf)
    job, rep = prover.prepare(pk, stdin)
    n = prover.job_shards(job)
    end = prover.job_snapshot(pk, job, capi.SNAP_EXIT)["summary"]
    row = dict(workload=name, cycles=int(rep["cycles"]), shards=n, calls=[])
    places = [("middle", ((n + 1) // 2, (end["row"] if n == 1 else 1 << 21) // 2)), ("exit", capi.SNAP_EXIT)]
    # beside a0, the register whose slice from the exit takes the most passes: what a long search costs
    widest = max(range(1, 32), key=lambda k: prover.job_origin(pk, job, capi.SNAP_EXIT, capi.origin_reg(k))["summary"]["passes"])
    for label, at, reg in [(label, at, reg) for reg in dict.fromkeys(("a0", capi.REG_NAMES[widest])) for label, at in places]:
        snap_reduce = []
        for _ in range(reps):
            prover.job_snapshot(pk, job, at)
            snap_reduce.append(round(prover.job_snapshot_times()["reduce_ms"], 3))
        for depth in (8, 64):
            out = dict(at=label, reg=reg, depth=depth, ms=[], reduce_ms=[], gather_ms=[], host_ms=[], snapshot_reduce_ms=snap_reduce)
            for _ in range(reps):
                got = prover.job_origin(pk, job, at, capi.origin_reg(reg), depth=depth)
                t = prover.job_origin_times()
                out["ms"].append(round(got["summary"]["ms"], 3))
                for k in ("reduce_ms", "gather_ms", "host_ms"):
                    out[k].append(round(t[k], 3))
            s = got["summary"]
            assert s["cycles"] == rep["cycles"]
            out.update({k: s[k] for k in ("position", "n_nodes", "n_edges", "cut", "unexpanded", "initial", "no_value", "questions", "levels", "passes")})
            out["reached"] = s["depth"]
            out["reduce_ms_per_pass"] = [round(v / max(s["passes"], 1), 3) for v in out["reduce_ms"]]
            row["calls"].append(out)
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
