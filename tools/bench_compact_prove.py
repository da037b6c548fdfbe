"""prove_core of bench.py's default job with "compact_openings" 0 and 1, in alternating pairs on two handles of one process.

  python tools/bench_compact_prove.py [--pairs 3] [--calls 3] [--device 0]

One JSON line: per pair the median wall time of each setting and its spread, the proof bytes of both forms, and whether the
compact prover's bytes equal capi.proof_compact of the plain proof."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    buf = bench.workload_stdin(0)
    elf = guests.dkg_like("finalization", *bench.fit_constants(buf, 32), **bench.guest_kw())
    handles = [capi.Prover({"device": args.device, "fri_queries": 100, "pow_bits": 16, "compact_openings": c}) for c in (0, 1)]
    keys = [p.setup(elf) for p in handles]
    proofs = [p.prove_core(pk, [buf])[0] for p, (pk, _) in zip(handles, keys)]   # (and warms both)
    vk = keys[0][1]
    out = {"plain_bytes": len(proofs[0]), "compact_bytes": len(proofs[1]), "ratio": round(len(proofs[1]) / len(proofs[0]), 4),
           "compact_prover_equals_transcoder": capi.proof_compact(vk, proofs[0]) == proofs[1], "pairs": []}
    for _ in range(args.pairs):
        row = {}
        for name, p, (pk, _) in zip(("plain", "compact"), handles, keys):
            ms = []
            for _ in range(args.calls):
                t = time.perf_counter()
                p.prove_core(pk, [buf])
                ms.append((time.perf_counter() - t) * 1e3)
            row[name + "_ms"] = round(statistics.median(ms), 1)
            row[name + "_spread_ms"] = round(max(ms) - min(ms), 1)
        out["pairs"].append(row)
    for p, (pk, _) in zip(handles, keys):
        p.pk_free(pk)
        p.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
