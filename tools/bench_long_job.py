#!/usr/bin/env python3
"""Long jobs under a prover config given on the command line: what bench.py, which takes no config, cannot measure.

Proves the dkg_like guest that bench.py builds for --shards N shards of 2^21 cycles, once per --cfg (a JSON object for
capi.Prover, e.g. '{"keep_phase1": 2}'), in --rounds alternating rounds.  Every (round, config) runs in a fresh child
process (this file again, with --child) under its own time limit; the parent never opens the GPU, and the first child that
fails or runs out of time ends the run.  A call is prepare (executor, uploads, phase 1) + prove_job (phase 2) + job_free.

Prints one JSON line: per config the ms per call of every round, their mean and spread (max - min over the rounds), guest
cycles per second, the shards per tier (dvt_rv32_job_shard_kept), the lowest free HBM seen after a prepare and whether
capi.verify accepted the last proof.

    python tools/bench_long_job.py --shards 32 --rounds 3 --cfg '{}' --cfg '{"keep_phase1": 2, "keep_full_max": 0}' --cfg '{"keep_phase1": 0}'
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TIERS = ("none", "tree", "full")


def child(args):
    """one config in this process: warm-up calls, timed calls, then one call whose proof is verified on the host"""
    import torch

    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    consts = tuple(int(x) for x in args.consts.split(","))
    stdin_buf = bench.workload_stdin()
    elf = guests.dkg_like("finalization", *consts, **bench.guest_kw())
    cfg = json.loads(args.child)
    p = capi.Prover(json.dumps(cfg))
    device = p.lib.dvt_prover_device(p.h, 0)
    pk, vk = p.setup(elf)
    seen = dict(min_free=None, tiers=None, cycles=0, shards=0)

    def call(want_bytes):
        job, rep = p.prepare(pk, [stdin_buf])
        free = int(torch.cuda.mem_get_info(device)[0])
        seen["min_free"] = free if seen["min_free"] is None else min(seen["min_free"], free)
        n = p.job_shards(job)
        kept = [p.job_shard_kept(job, i) for i in range(n)]
        seen.update(tiers={name: kept.count(t) for t, name in enumerate(TIERS)}, cycles=int(rep["cycles"]), shards=n)
        out = p.prove_job(pk, job, want_bytes=want_bytes)
        p.job_free(job)
        return out

    for _ in range(args.warmup):
        call(False)
    p.sync()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        call(False)
        p.sync()
        times.append((time.perf_counter() - t0) * 1e3)
    verified = None
    if not args.no_verify:
        proof = call(True)
        ok, ec, pv, why = capi.verify(vk, proof, int(cfg.get("fri_queries", 100)), int(cfg.get("pow_bits", 16)))
        want = guests.dkg_like_expected(stdin_buf, "finalization", *consts, curve_precompiles=bench.CURVE_PRECOMPILES)
        verified = bool(ok and ec == 0 and pv == want)
    p.pk_free(pk)
    p.close()
    ms = sum(times) / len(times)
    print(json.dumps(dict(cfg=cfg, ms_per_call=round(ms, 2), calls_ms=[round(t, 2) for t in times], cycles=seen["cycles"], shards=seen["shards"],
                          cycles_per_s=round(seen["cycles"] / (ms / 1e3)), tiers=seen["tiers"], min_free_bytes=seen["min_free"], verified=verified)))
    return 0 if verified is not False else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shards", type=int, default=32, help="shards of 2^21 cycles of the execution")
    ap.add_argument("--cfg", action="append", default=[], help="a prover config (JSON object); may repeat")
    ap.add_argument("--rounds", type=int, default=1, help="every config once per round, in the order given")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one (round, config) may take")
    ap.add_argument("--no-verify", action="store_true", help="skip the verified extra call (very long jobs)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--consts", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)

    import bench   # (host only here: the guest is executed, never proven, in this process)

    cfgs = [json.loads(c) for c in (args.cfg or ["{}"])]
    for c in cfgs:
        if not isinstance(c, dict):
            ap.error("--cfg takes a JSON object")
    consts = bench.fit_constants(bench.workload_stdin(), args.shards)
    runs = [[] for _ in cfgs]
    failed = None
    for r in range(args.rounds):
        for k, c in enumerate(cfgs):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(c), "--consts", ",".join(str(x) for x in consts),
                   "--steps", str(args.steps), "--warmup", str(args.warmup)] + (["--no-verify"] if args.no_verify else [])
            try:
                done = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.timeout, cwd=ROOT)
                lines = [ln for ln in done.stdout.decode().splitlines() if ln.startswith("{")]
                if lines:
                    runs[k].append(json.loads(lines[-1]))
                if done.returncode or not lines:
                    failed = dict(round=r, cfg=c, returncode=done.returncode)
            except subprocess.TimeoutExpired:
                failed = dict(round=r, cfg=c, returncode=None, timeout_s=args.timeout)
            if failed:
                break
        if failed:
            break
    out = []
    for c, rs in zip(cfgs, runs):
        ms = [x["ms_per_call"] for x in rs]
        row = dict(cfg=c, rounds_ms=ms)
        if rs:
            mean = sum(ms) / len(ms)
            row.update(ms_per_call=round(mean, 2), spread_ms=round(max(ms) - min(ms), 2), cycles=rs[-1]["cycles"], shards=rs[-1]["shards"],
                       cycles_per_s=round(rs[-1]["cycles"] / (mean / 1e3)), tiers=rs[-1]["tiers"],
                       min_free_bytes=min(x["min_free_bytes"] for x in rs), verified=rs[-1]["verified"])
        out.append(row)
    print(json.dumps(dict(shards=args.shards, steps=args.steps, warmup=args.warmup, rounds=args.rounds, consts=list(consts), configs=out, failed=failed)))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
