"""Host verifier against device verifier on the same proof bytes: capi.verify (one host thread) and Prover.verify (the
query part on the GPU), in alternating pairs.

  python tools/bench_verify.py [--pairs 3] [--calls 5] [--jobs default,reference,n255] [--compact]

One JSON line per job: the medians per pair, the host call's run-to-run spread, the split of the device call (host part /
flatten / upload / kernels / download / waiting) and the Poseidon2 permutation count.  The jobs: bench.py's default
container (32 shards of 2^21 cycles), the reference example (one short, wide shard: tools/bench_reference_guest.py) and
the --participants 255 --sha-precompiles --curve-precompiles job of bench.py.  With --compact the proof is turned into the
compact form first (capi.proof_compact; "plain_bytes" is the size it had): the same job in both forms is two runs."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_job(name, prover):
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    if name == "reference":
        from tests import guests_finalization as gf

        buf = capi.stdin_from_json("finalization", open(os.path.join(ROOT, "tests", "golden", "finalization_example.json"), "rb").read())
        elf = gf.finalization(nmax=8, kmax=8)
    else:
        wide = name == "n255"
        bench.SHA_PRECOMPILES = bench.CURVE_PRECOMPILES = wide
        buf = bench.workload_stdin(255 if wide else 0)
        elf = guests.dkg_like("finalization", *bench.fit_constants(buf, 32), **bench.guest_kw())
    pk, vk = prover.setup(elf)
    proof, rep = prover.prove_core(pk, [buf])
    prover.pk_free(pk)
    return vk, proof, rep


def measure(name, prover, pairs, calls, compact=False):
    from dvt_circuits_amd import capi

    vk, proof, rep = make_job(name, prover)
    plain_bytes = len(proof)
    if compact:
        plain = proof
        proof = capi.proof_compact(vk, plain)
        assert capi.verify(vk, proof) == capi.verify(vk, plain) and capi.proof_expand(vk, proof) == plain
    assert prover.verify(vk, proof) == capi.verify(vk, proof) and capi.verify(vk, proof)[0]   # (and warms both paths)
    out = {"job": name, "shards": len(capi.split_container(proof)[2]), "proof_bytes": len(proof), "plain_bytes": plain_bytes, "compact": compact, "cycles": rep["cycles"], "pairs": []}
    for _ in range(pairs):
        host, dev, split = [], [], []
        for _ in range(calls):
            t = time.perf_counter()
            capi.verify(vk, proof)
            host.append((time.perf_counter() - t) * 1e3)
        for _ in range(calls):
            t = time.perf_counter()
            prover.verify(vk, proof)
            dev.append((time.perf_counter() - t) * 1e3)
            split.append(prover.verify_times())
        mid = sorted(range(calls), key=lambda i: dev[i])[calls // 2]
        out["pairs"].append({"host_ms": round(statistics.median(host), 2), "host_spread_ms": round(max(host) - min(host), 2),
                             "device_ms": round(statistics.median(dev), 2), "device_spread_ms": round(max(dev) - min(dev), 2),
                             "device_split": {k: round(v, 3) for k, v in split[mid].items()}})
    out["permutations"] = int(out["pairs"][0]["device_split"]["permutations"])
    out["device_wins_every_pair_by_twice_the_host_spread"] = all(p["host_ms"] - p["device_ms"] > 2 * p["host_spread_ms"] for p in out["pairs"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--jobs", default="default,reference,n255")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--compact", action="store_true")
    args = ap.parse_args()
    from dvt_circuits_amd import capi

    for name in args.jobs.split(","):
        prover = capi.Prover('{"device": %d, "fri_queries": 100, "pow_bits": 16}' % args.device)
        print(json.dumps(measure(name, prover, args.pairs, max(5, args.calls), args.compact)), flush=True)
        prover.close()


if __name__ == "__main__":
    main()
