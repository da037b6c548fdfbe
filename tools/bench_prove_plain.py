"""One process, one build: prove_core of bench.py's default job (default config, plain proofs) and Prover.verify of its proof.

  python tools/bench_prove_plain.py [--root DIR] [--calls 3] [--device 0]

--root names the checkout to import from (this one by default), so that two builds, such as a commit and its parent, can be
measured in alternating processes of one job.  It uses nothing a build from before the compact proof form lacks.  One JSON
line: the median and spread of the prove calls (after one warming call) and of the device verify calls, the verify split,
and the SHA-256 of the proof bytes."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    os.chdir(root)
    import bench
    from dvt_circuits_amd import capi
    from tests import guests

    assert os.path.abspath(capi.__file__).startswith(root + os.sep), capi.__file__
    buf = bench.workload_stdin(0)
    elf = guests.dkg_like("finalization", *bench.fit_constants(buf, 32), **bench.guest_kw())
    p = capi.Prover('{"device": %d, "fri_queries": 100, "pow_bits": 16}' % args.device)
    pk, vk = p.setup(elf)
    proof, _ = p.prove_core(pk, [buf])
    prove = []
    for _ in range(args.calls):
        t = time.perf_counter()
        p.prove_core(pk, [buf])
        prove.append((time.perf_counter() - t) * 1e3)
    assert p.verify(vk, proof)[0]
    ver, split = [], []
    for _ in range(max(5, args.calls)):
        t = time.perf_counter()
        p.verify(vk, proof)
        ver.append((time.perf_counter() - t) * 1e3)
        split.append(p.verify_times())
    mid = sorted(range(len(ver)), key=lambda i: ver[i])[len(ver) // 2]
    p.pk_free(pk)
    p.close()
    print(json.dumps({"root": root, "prove_ms": round(statistics.median(prove), 1), "prove_spread_ms": round(max(prove) - min(prove), 1),
                      "verify_ms": round(statistics.median(ver), 2), "verify_spread_ms": round(max(ver) - min(ver), 2),
                      "verify_split": {k: round(v, 3) for k, v in split[mid].items()}, "proof_bytes": len(proof),
                      "proof_sha256": hashlib.sha256(proof).hexdigest()}), flush=True)


if __name__ == "__main__":
    main()
