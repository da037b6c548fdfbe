#!/usr/bin/env python3
"""What a uses slice costs beside an origin slice and the memory report, on one GPU in one process.

    python tools/bench_uses.py [--shards 32] [--reps 5] [--out FILE.jsonl]

On the dkg_like job of tools/bench_origin.py (--shards shards of 2^21 cycles) four calls, after one warm-up each, --reps
repetitions: `first`: the register with the most uses from the first record on (all 31 are asked), depth 0 (one definition, the
longest suffix); `middle`: the same from the middle; `loop`: that register from the middle to the caps (depth 64, fan 16,
addresses followed); `store`: the word of the first store in the loop call's slice, three levels deep (left out when the slice
has no store); `live_first` / `live_middle`: sp with depth 0, a definition nothing overwrites, so that the count and scan passes run
over every span behind the position.  Per call one JSON line: every repetition's summary["ms"] (milliseconds inside the
library after the entry guard: uploads, downloads and the host's search included) and the next, count + scan, emit and gather
launches as stream events time them, summed over the levels and passes of the call (Prover.job_uses_times), with the passes, so
that next_ms / passes and count_ms / passes are one pass over the records of the windows; median and spread (min, max) of each.
Beside them, measured in the same run on the same job: Prover.job_origin of a0 at the exit (reduce_ms / passes: one origin pass
over all records) and the wall clock of Prover.job_memory."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values):
    return dict(median=round(statistics.median(values), 3), min=round(min(values), 3), max=round(max(values), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shards", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    example = bench.workload_stdin()
    consts = bench.fit_constants(example, args.shards)
    elf = guests.dkg_like("finalization", *consts, **bench.guest_kw())
    prover = capi.Prover('{"device": 0, "fri_queries": 100, "pow_bits": 16, "log_shard_size": 21}')
    pk, _ = prover.setup(elf)
    job, rep = prover.prepare(pk, [example])
    n = prover.job_shards(job)
    middle = ((n + 1) // 2, (1 << 21) // 2 if n > 1 else int(rep["cycles"]) // 2)
    lines = []

    def emit(row):
        print(json.dumps(row), flush=True)
        lines.append(row)
        if args.out:   # (written as it goes: a later call that fails keeps the earlier lines)
            with open(args.out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")

    # the yardsticks, in the same run on the same job
    origin = dict(ms=[], reduce_ms=[], reduce_ms_per_pass=[])
    for k in range(args.reps + 1):
        got = prover.job_origin(pk, job, capi.SNAP_EXIT, capi.origin_reg("a0"))
        t = prover.job_origin_times()
        if k:
            origin["ms"].append(got["summary"]["ms"])
            origin["reduce_ms"].append(t["reduce_ms"])
            origin["reduce_ms_per_pass"].append(t["reduce_ms"] / max(got["summary"]["passes"], 1))
    memory = []
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        prover.job_memory(pk, job)
        if k:
            memory.append(1000 * (time.perf_counter() - t0))
    emit(dict(workload="dkg_like%r" % (consts,), cycles=int(rep["cycles"]), shards=n, reps=args.reps, origin_a0_exit_passes=got["summary"]["passes"],
              origin_a0_exit={k: spread(v) for k, v in origin.items()}, memory_wall_ms=spread(memory)))
    # the register with the most uses from each position (all 31 are asked, as tools/bench_origin.py picks its register); the
    # store: the first STORE consumer in the loop call's slice
    def busiest(at):
        return max(range(1, 32), key=lambda k: prover.job_uses(pk, job, at, capi.uses_reg(k), depth=0, follow_addr=True)["defs"][0]["n_uses"])

    r_first, r_middle = busiest((1, 0)), busiest(middle)
    loop_kw = dict(depth=64, fan=16, follow_addr=True)
    probe = prover.job_uses(pk, job, middle, capi.uses_reg(r_middle), **loop_kw)
    store = next((x for x in probe["nodes"] if x["kind"] == capi.DVT_USES_STORE), None)
    calls = [("first", (1, 0), capi.uses_reg(r_first), dict(depth=0, follow_addr=True)), ("middle", middle, capi.uses_reg(r_middle), dict(depth=0, follow_addr=True)),
             ("loop", middle, capi.uses_reg(r_middle), loop_kw)]
    # sp is never written again in this guest: its window is the whole suffix, so count and scan run over every span behind the position
    calls += [("live_first", (1, 0), capi.uses_reg("sp"), dict(depth=0, follow_addr=True)), ("live_middle", middle, capi.uses_reg("sp"), dict(depth=0, follow_addr=True))]
    if store:
        calls.insert(2, ("store", (store["shard"], store["row"] + 1), capi.uses_word(store["addr"]), dict(depth=3)))
    for label, at, target, kw in calls:
        keys = ("next_ms", "count_ms", "emit_ms", "gather_ms", "host_ms")
        out = dict(ms=[], **{k: [] for k in keys})
        for k in range(args.reps + 1):
            got = prover.job_uses(pk, job, at, target, **kw)
            t = prover.job_uses_times()
            if k:
                out["ms"].append(got["summary"]["ms"])
                for key in keys:
                    out[key].append(t[key])
        s = got["summary"]
        row = dict(call=label, at=list(at), target=list(target), reg=capi.REG_NAMES[target[1]] if target[0] == capi.DVT_USES_REG else None,
                   **{k: int(v) for k, v in kw.items()})
        row.update({k: s[k] for k in ("position", "n_nodes", "n_defs", "n_edges", "depth", "cut", "unexpanded", "truncated", "dead", "live_at_exit", "uses_total",
                                      "levels", "passes")})
        row.update({k: spread(v) for k, v in out.items()})
        row["next_ms_per_pass"] = round(statistics.median(out["next_ms"]) / max(s["passes"], 1), 3)
        row["count_ms_per_pass"] = round(statistics.median(out["count_ms"]) / max(s["passes"], 1), 3)
        emit(row)
    prover.job_free(job)
    prover.pk_free(pk)
    prover.close()


if __name__ == "__main__":
    main()
